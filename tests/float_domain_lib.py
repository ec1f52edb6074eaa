"""The float-PCM engines at the edges of the float domain (TEST INFRASTRUCTURE: nothing under atracdenc_amd/ imports this).

One table of named patterns. A pattern is a function that writes into block 3 (1024 stereo samples) of an otherwise ordinary
stream, SIGNALS["mix"] over 12 blocks: the blocks before it fill the carried state, the blocks after it show the recovery.
The same 12 blocks are every other layout too: 24 ATRAC1 blocks of 512, 6 ATRAC3plus frames of 2048 (mono and stereo), and
one flat [T][C] stream for the resampler, the meter and the limiter. The ATRAC3plus tone analysis takes the 6 frames too.

Used by tests/test_float_domain_cpu.py (oracle and restatements, sanitized, and the oracle against the reference build), by
the `domain` family of the tools/emu drivers (kernel sources on the CPU) and by tests/test_float_domain_gpu.py.
"""
import numpy as np

from at3_testlib import SIGNALS

N_BLOCKS = 12
BAD_BLOCK = 3
FLT_MAX = np.float32(3.4028234663852886e38)
NAN = np.float32(np.nan)
INF = np.float32(np.inf)


def _bits(*words):
    return np.array(words, np.uint32).view(np.float32)


def _clean(b):
    pass


def _nan1(b):
    b[500, 0] = NAN


def _inf_pair(b):
    b[500, 0] = INF
    b[502, 0] = -INF


def _max1(b):
    b[500, 0] = FLT_MAX


def _nan_block(b):
    b[:] = NAN


def _max_alt(b):
    # +MAX +MAX -MAX -MAX ...: finite input whose filter sums overflow, so that inf - inf appears inside the engines
    b[:] = np.where((np.arange(1024) // 2) % 2 == 0, FLT_MAX, -FLT_MAX).astype(np.float32)[:, None]


def _inf_left(b):
    b[:, 0] = INF


def _mixed(b):
    f = b.reshape(-1)
    f[::7] = -INF
    f[::5] = NAN


def _nan_bits(b):
    # a signalling NaN, a negative quiet NaN with a payload, and the all-ones positive NaN, as bit patterns
    b[100, 0], b[101, 1], b[600, 0] = _bits(0x7FA00000, 0xFFC00001, 0x7FFFFFFF)


def _e19_alt(b):
    # a square is 1e38: an f32 energy sum overflows with the fourth sample, an f64 one never
    b[:] = np.where(np.arange(1024) % 2 == 0, 1e19, -1e19).astype(np.float32)[:, None]


def _e15(b):
    # every intermediate stays finite: 1e15^2 * 1024 = 1e33
    b[:] = (np.random.RandomState(15).uniform(-1.0, 1.0, b.shape) * 1e15).astype(np.float32)


def _subnormal(b):
    k = np.random.RandomState(42).randint(-200, 201, b.shape)
    v = (k.astype(np.float64) * 1e-42).astype(np.float32)     # multiples of 1e-42: all subnormal (|v| <= 2e-40)
    v[k == 0] = np.float32(-0.0)
    v[::2][k[::2] == 0] = np.float32(0.0)
    b[:] = v


PATTERNS = {
    "clean": _clean,
    "nan1": _nan1,
    "inf_pair": _inf_pair,
    "max1": _max1,
    "nan_block": _nan_block,
    "max_alt": _max_alt,
    "inf_left": _inf_left,
    "mixed": _mixed,
    "nan_bits": _nan_bits,
    "e19_alt": _e19_alt,
    "e15": _e15,
    "subnormal": _subnormal,
}
NAMES = tuple(PATTERNS)
# finite input for which the oracle's damage is bounded: parity on these has no exceptions
COMPULSORY = ("clean", "e15", "subnormal", "max1")

# The one exception table: (engine, pattern) -> reason. An entry replaces bit parity for that stream by the weaker contract of
# tests/test_float_domain_gpu.py (the call succeeds, the result repeats, every other stream equals its oracle, the stream
# equals the oracle again once the oracle equals its own clean encode). Engines: "at3", "at1", "at3p", "resample", "loudness",
# "limiter" (the look-ahead limiter) and "tones" (the ATRAC3plus tone analysis: at3phip_analyse_tones, at3phip_encode_frames_tonal).
EXCEPTIONS = {}
assert not any(p in COMPULSORY for _, p in EXCEPTIONS)

_base = {}


def stream(name, n_blocks=N_BLOCKS):
    """float32 [n_blocks, 1024, 2]: the ordinary stream with block 3 rewritten by pattern `name`"""
    if n_blocks not in _base:
        _base[n_blocks] = SIGNALS["mix"](n_blocks)
        _base[n_blocks].setflags(write=False)
    x = _base[n_blocks].copy()
    PATTERNS[name](x[BAD_BLOCK])
    return x


def at3_batch(names=NAMES):
    """[len(names), 12, 1024, 2]"""
    return np.stack([stream(n) for n in names])


def at1_batch(nch, names=NAMES):
    """[len(names), 24, 512, nch]"""
    return np.stack([np.ascontiguousarray(stream(n).reshape(-1, 512, 2)[:, :, :nch]) for n in names])


def at3p_batch(nch, names=NAMES):
    """[len(names), 6, 2048, nch]"""
    return np.stack([np.ascontiguousarray(stream(n).reshape(-1, 2048, 2)[:, :, :nch]) for n in names])


def flat_batch(nch, T=N_BLOCKS * 1024, names=NAMES):
    """[len(names), T, nch]: the first T samples of each stream (of as many blocks as T needs); the pattern is samples 3072 .. 4095"""
    return np.stack([np.ascontiguousarray(stream(n, max(N_BLOCKS, -(-T // 1024))).reshape(-1, 2)[:T, :nch]) for n in names])


def floats_match(got, exp):
    """Float outputs are compared as bit patterns where the expectation is finite or infinite; where it is a NaN the
    result must be a NaN too, of any sign and payload (inf - inf is 0xFFC00000 on x86 and 0x7FC00000 on the GPU, and
    neither engine promises a payload). Returns the boolean mask of mismatching elements."""
    got, exp = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    assert got.shape == exp.shape and got.dtype == exp.dtype and got.dtype in (np.float32, np.float64), (got.shape, exp.shape, got.dtype)
    word = np.uint32 if got.dtype == np.float32 else np.uint64
    return np.where(np.isnan(exp), ~np.isnan(got), got.view(word) != exp.view(word))


def assert_floats_match(got, exp, what):
    bad = floats_match(got, exp)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} differ, first at {np.argwhere(bad)[:4].tolist()}"


def first_clean_frame(frames, clean_frames):
    """the first index from which `frames` (the oracle's, of a poisoned stream) equals its clean encode to the end"""
    diff = (frames != clean_frames).reshape(frames.shape[0], -1).any(axis=1)
    idx = np.nonzero(diff)[0]
    return 0 if idx.size == 0 else int(idx[-1]) + 1


# ---- one run of each engine on the batch, and its expectation ---------------------------------------------------------------
# The same functions serve the SIMT harness (lib_path = the harness library) and the GPU (lib_path = None). Every output
# is a host array filled with a sentinel before the call (0xA5 bytes, 0x5A5A samples, the float 0xA5A5A5A5), so a region
# that is never written cannot pass. The expectations are computed once per process and handed out read-only.
SENT_U8, SENT_S16, SENT_F32 = 0xA5, 0x5A5A, 0xA5A5A5A5
_memo = {}


def _once(key, fn):
    if key not in _memo:
        v = fn()
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _memo[key] = v
    return _memo[key]


def _sent(shape, dtype):
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return np.full(shape, SENT_F32, np.uint32).view(np.float32)
    return np.full(shape, SENT_S16 if dtype == np.int16 else SENT_U8, dtype)


def rows_bad(got, exp, engine, names, clean=None):
    """per-stream comparison of byte outputs [S][N]...: the names of the streams that break their contract. A stream whose
    (engine, pattern) is in EXCEPTIONS only has to equal `exp` from the first frame at which exp equals `clean` again."""
    assert got.shape == exp.shape and got.dtype == exp.dtype, (got.shape, exp.shape, got.dtype, exp.dtype)
    bad = []
    for i, n in enumerate(names):
        k = 0
        if (engine, n) in EXCEPTIONS:
            assert clean is not None
            k = first_clean_frame(exp[i], clean)
        if not np.array_equal(got[i, k:], exp[i, k:]):
            bad.append(n)
    return bad


AT3_SPLIT = (5, 1, 6)
# (bitrate, no_gain, no_tonal, channels, patterns): LP2 and LP4 with every tool and with none; LP4 from one channel (joint stereo)
AT3_CASES = ((132300, 0, 0, 2, NAMES), (132300, 1, 1, 2, NAMES), (66150, 0, 0, 2, NAMES), (66150, 1, 1, 2, NAMES),
             (66150, 0, 0, 1, ("clean", "nan1", "max_alt")))


def at3_run(lib_path, br, ng, nt, channels=2, names=NAMES, split=None):
    """(frames [S, 11, frame_size], (scale_overflow, clipped_values)) of one context over the batch, fed whole or as `split`"""
    from atracdenc_amd.binding import At3Hip
    pcm = np.ascontiguousarray(at3_batch(names)[..., :channels])
    S, nb = pcm.shape[:2]
    enc = At3Hip(n_streams=S, max_blocks=nb, bitrate=br, no_gain=ng, no_tonal=nt, channels=channels, lib_path=lib_path)
    try:
        fs, parts, at = enc.frame_size, [], 0
        for k in (split or (nb,)):
            piece = np.ascontiguousarray(pcm[:, at:at + k])
            out = _sent(S * k * fs, np.uint8)
            n = enc.encode_ptr(piece.ctypes.data, k, out.ctypes.data, 0)
            assert (out[S * n * fs:] == SENT_U8).all(), "bytes past the packed frames were written"
            parts.append(out[:S * n * fs].reshape(S, n, fs))
            at += k
        c = enc.counters()
    finally:
        enc.close()
    return np.concatenate(parts, axis=1), (c["scale_overflow"], c["clipped_values"])


def at3_expect(br, ng, nt, channels=2, names=NAMES):
    """(frames [S, 11, frame_size], per-stream (scale_overflow, clipped_values) [S, 2]) of the oracle, each stream alone"""
    from at3_testlib import oracle, oracle_diag_counts

    def make():
        o, frames, counts = oracle(), [], []
        oracle_diag_counts(reset=True)
        for n in names:
            frames.append(o.encode(np.ascontiguousarray(stream(n)[..., :channels]), br, ng, nt)[0])
            counts.append(oracle_diag_counts(reset=True))
        return np.stack(frames), np.array(counts, np.int64)
    return _once(("at3", br, ng, nt, channels, names), make)


AT1_SPLIT = (10, 2, 12)
AT1_CASES = (("auto", 2), ("auto", 1), ("short", 2), ("short", 1))   # (mode, channels)


def at1_run(lib_path, mode, nch, names=NAMES, split=None):
    """(sound units [S, 24, nch, 212], loudness tap [S, 24]) of one context"""
    from at3_testlib import AT1_MODES
    from atracdenc_amd.binding import At1Hip
    pcm = at1_batch(nch, names)
    S, nb = pcm.shape[:2]
    auto, mask, bfu = AT1_MODES[mode]
    enc = At1Hip(n_streams=S, max_blocks=nb, channels=nch, window_auto=auto, window_mask=mask, bfu_idx_const=bfu, lib_path=lib_path)
    try:
        units, loud, at = [], [], 0
        for k in (split or (nb,)):
            piece = np.ascontiguousarray(pcm[:, at:at + k])
            out = _sent((S, k, nch, 212), np.uint8)
            enc.encode_ptr(piece.ctypes.data, k, out.ctypes.data, 0)
            units.append(out)
            loud.append(enc.read_tap(At1Hip.TAP_LOUDNESS, np.float32, (S, k)))
            at += k
    finally:
        enc.close()
    return np.concatenate(units, axis=1), np.concatenate(loud, axis=1)


def at1_expect(mode, nch, names=NAMES):
    from at3_testlib import at1_oracle_encode

    def make():
        e = [at1_oracle_encode(p, mode, taps=True) for p in at1_batch(nch, names)]
        return np.stack([x[0] for x in e]), np.stack([x[3] for x in e])
    return _once(("at1", mode, nch, names), make)


AT3P_SPLIT = (2, 1, 3)


def at3p_run(lib_path, nch, names=NAMES, split=None):
    """frames [S, 6, 2048] of encode_frames"""
    from atracdenc_amd.binding import At3pHip
    pcm = at3p_batch(nch, names)
    S, nf = pcm.shape[:2]
    enc = At3pHip(n_streams=S, max_frames=nf, channels=nch, lib_path=lib_path)
    try:
        parts, at = [], 0
        for k in (split or (nf,)):
            piece = np.ascontiguousarray(pcm[:, at:at + k])
            out = _sent((S, k, 2048), np.uint8)
            enc.encode_frames_ptr(piece.ctypes.data, k, out.ctypes.data, 0)
            parts.append(out)
            at += k
    finally:
        enc.close()
    return np.concatenate(parts, axis=1)


def at3p_expect(nch, names=NAMES):
    """the oracle's PQF -> division by 32768 / 1.122018 -> MDCT -> frame writer, each stream alone"""
    from at3_testlib import at3p_mdct, at3p_pqf, at3p_write_frames

    def make():
        frames = []
        for pcm in at3p_batch(nch, names):
            specs = np.zeros((pcm.shape[0], nch, 2048), np.float32)
            for c in range(nch):
                bands = at3p_pqf(np.ascontiguousarray(pcm[:, :, c]))
                with np.errstate(all="ignore"):
                    bands = (bands.astype(np.float64) / (32768.0 / 1.122018)).astype(np.float32)
                specs[:, c] = at3p_mdct(bands)
            frames.append(at3p_write_frames(specs))
        return np.stack(frames)
    return _once(("at3p", nch, names), make)


RESAMPLE_T = 3001
RESAMPLE_PAIRS = ((48000, 44100), (44100, 48000))


RESAMPLE_CUTS = (700, 1500, RESAMPLE_T)


def resample_batch(nch, names=NAMES):
    """[S, 3001, nch]: samples 2048 .. 5048 of each stream, so that the whole bad block (1024 .. 2047 here) and the recovery lie inside"""
    return np.ascontiguousarray(flat_batch(nch, names=names)[:, 2048:2048 + RESAMPLE_T])


def s16_of(x):
    """the resampler's 16-bit form: lrintf(clamp(x, -1, 1) * 32767) as int16; a NaN passes the clamp and converts to 0"""
    with np.errstate(all="ignore"):
        y = np.where(x < -1.0, np.float32(-1.0), np.where(x > 1.0, np.float32(1.0), x)).astype(np.float32) * np.float32(32767.0)
        return np.where(np.isnan(y), 0, np.rint(np.nan_to_num(y))).astype(np.int16)


def resample_run(lib_path, pair, nch, s16, names=NAMES, cuts=(RESAMPLE_T,)):
    """the converted streams [S, n_out, nch] (float32 or int16): calls ending at `cuts`, then the flush"""
    from atracdenc_amd.binding import AT3HIP_RESAMPLE_OUT_S16, HipResampler
    xs = resample_batch(nch, names)
    S = xs.shape[0]
    r = HipResampler(*pair, channels=nch, n_streams=S, max_in=RESAMPLE_T, lib_path=lib_path)
    try:
        parts, at = [], 0
        flags = AT3HIP_RESAMPLE_OUT_S16 if s16 else 0
        for cut in tuple(cuts) + (None,):
            out = _sent((S * r.max_out * nch,), np.int16 if s16 else np.float32)
            if cut is None:
                n = r.flush_ptr(out.ctypes.data, flags)
            else:
                piece = np.ascontiguousarray(xs[:, at:cut])
                n = r.process_ptr(piece.ctypes.data, cut - at, out.ctypes.data, flags)
                at = cut
            rest = out[S * n * nch:]
            assert (rest.view(np.uint32) == SENT_F32).all() if not s16 else (rest == SENT_S16).all(), "samples past the outputs were written"
            parts.append(out[:S * n * nch].reshape(S, n, nch))
    finally:
        r.close()
    return np.concatenate(parts, axis=1)


def resample_expect(pair, nch, names=NAMES):
    """float32 [S, n_out, nch] of tests/host/resample_cpu.c, each stream alone"""
    from resample_lib import CpuResampler
    return _once(("resample", pair, nch, names), lambda: np.stack([CpuResampler(*pair, nch).whole(x) for x in resample_batch(nch, names)]))


def resample_bad(got, exp, s16, names=NAMES):
    """the names of the streams whose output differs from the restatement's (16-bit: exactly; float: floats_match)"""
    want = s16_of(exp) if s16 else exp
    if got.shape != want.shape:
        return list(names)
    return [n for i, n in enumerate(names) if ("resample", n) not in EXCEPTIONS and
            (not np.array_equal(got[i], want[i]) if s16 else floats_match(got[i], want[i]).any())]


METER_T = 52920   # 1.2 s: 12 hops
METER_CUTS = (3500, 4410 * 2 + 1, METER_T)


def meter_run(lib_path, nch, names=NAMES, cuts=(METER_T,)):
    """(hop sums float64 [S, 12, nch], results, apply's output [S, T, nch]) of one meter with true peak on"""
    from atracdenc_amd.binding import HipLoudness
    xs = flat_batch(nch, METER_T, names)
    S = xs.shape[0]
    m = HipLoudness(channels=nch, n_streams=S, max_in=METER_T, max_hops=METER_T // 4410, true_peak=True, lib_path=lib_path)
    try:
        at = 0
        for cut in cuts:
            m.process(xs[:, at:cut])
            at = cut
        z = m.hops()
        res = m.finish()
        out = _sent(xs.shape, np.float32)
        m.apply_ptr(xs.ctypes.data, METER_T, meter_gains(S), out.ctypes.data, 0)
    finally:
        m.close()
    return z, res, out


def meter_gains(S):
    return (np.float32(0.25) + np.arange(S, dtype=np.float32) * np.float32(0.37)).astype(np.float32)


def meter_expect(nch, names=NAMES):
    """(hops, results, scaled samples) of tests/host/loudness_cpu.c and numpy's float32 multiply, each stream alone"""
    import loudness_lib as L

    def make():
        xs = flat_batch(nch, METER_T, names)
        with np.errstate(all="ignore"):
            scaled = xs * meter_gains(xs.shape[0])[:, None, None]
        return np.stack([L.hops(x) for x in xs]), [L.measure(x, True) for x in xs], scaled
    return _once(("meter", nch, names), make)


def result_mismatch(got, exp):
    """the names of the fields of an at3hip_loudness_result that differ: integers exactly, floats by floats_match's rule"""
    import loudness_lib as L
    bad = []
    for f in L.FIELDS:
        a, b = getattr(got, f), getattr(exp, f)
        if f in ("sample_peak", "true_peak"):
            ok = not floats_match(np.array(a[:], np.float32), np.array(b[:], np.float32)).any()
        elif f in ("integrated", "momentary_max", "short_term_max"):
            ok = not floats_match(np.array([a], np.float64), np.array([b], np.float64)).any()
        else:
            ok = int(a) == int(b)
        if not ok:
            bad.append(f)
    return bad


def meter_bad(got, exp, names=NAMES):
    """{"z" | "results" | "apply": the names of the streams that differ from the restatement}"""
    (z, res, out), (ez, eres, eout) = got, exp
    live = [(i, n) for i, n in enumerate(names) if ("loudness", n) not in EXCEPTIONS]
    return {"z": [n for i, n in live if floats_match(z[i], ez[i]).any()],
            "results": [f"{n}:{','.join(result_mismatch(res[i], eres[i]))}" for i, n in live if result_mismatch(res[i], eres[i])],
            "apply": [n for i, n in live if floats_match(out[i], eout[i]).any()]}


LIMITER_T = 6000
LIMITER_CUTS = (3100, 3100 + 71, LIMITER_T)
TINY = np.float32(1.4e-45)                     # the smallest subnormal
LIMITER_CEIL = np.float32(10.0 ** (-1.0 / 20.0))   # -1 dBFS (limiter_lib.CEIL)
# (gain, ceiling): no gain, an ordinary one, one whose every product overflows, the smallest and the largest ceiling, the smallest gain
LIMITER_PAIRS = ((np.float32(0.0), LIMITER_CEIL), (np.float32(2.0), LIMITER_CEIL), (FLT_MAX, LIMITER_CEIL),
                 (np.float32(2.0), TINY), (np.float32(2.0), FLT_MAX), (TINY, LIMITER_CEIL))
LIMITER_CEILINGS = tuple(dict.fromkeys(c for _, c in LIMITER_PAIRS))


def limiter_streams(nch, ceiling, names=NAMES):
    """(xs [S, 6000, nch], gains [S], labels [S]) of the run with this ceiling: the gain is per stream and the ceiling per run, so
    flat_batch() is repeated once for every gain that LIMITER_PAIRS pairs with the ceiling"""
    gains = [g for g, c in LIMITER_PAIRS if c == ceiling]
    assert gains, ceiling
    one = flat_batch(nch, LIMITER_T, names)
    xs = np.ascontiguousarray(np.concatenate([one] * len(gains)))
    return xs, np.repeat(np.array(gains, np.float32), len(names)), [f"{n}@g={float(g):g}" for g in gains for n in names]


def limiter_run(lib_path, nch, true_peak, ceiling, names=NAMES, cuts=(LIMITER_T,)):
    """(samples [S, 6000, nch], [(min S, limited count)] per stream) of one limiter run: calls ending at `cuts`, then the flush"""
    from atracdenc_amd.binding import HipLoudness
    xs, gains, _ = limiter_streams(nch, ceiling, names)
    S, T = xs.shape[:2]
    m = HipLoudness(channels=nch, n_streams=S, max_in=T, max_hops=1, lib_path=lib_path)
    try:
        m.limit_start(gains, ceiling, true_peak)
        parts, at = [], 0
        for cut in tuple(cuts) + (None,):
            out = _sent((S * T * nch,), np.float32)
            if cut is None:
                n = m.limit_flush_ptr(out.ctypes.data, 0)
            else:
                piece = np.ascontiguousarray(xs[:, at:cut])
                n = m.limit_ptr(piece.ctypes.data, cut - at, out.ctypes.data, 0)
                at = cut
            assert (out[S * n * nch:].view(np.uint32) == SENT_F32).all(), "samples past the outputs were written"
            parts.append(out[:S * n * nch].reshape(S, n, nch))
        st = m.limit_stats()
        assert all(s.n_out == T for s in st), [s.n_out for s in st]
    finally:
        m.close()
    return np.concatenate(parts, axis=1), [(s.min_sum, s.n_limited) for s in st]


def limiter_expect(nch, true_peak, ceiling, names=NAMES):
    """(samples [S, 6000, nch], [(min S, limited count)]) of tests/host/limiter_cpu.c, each stream alone"""
    import limiter_lib as LM

    def make():
        xs, gains, _ = limiter_streams(nch, ceiling, names)
        return LM.restate_all(xs, gains, ceiling, true_peak)
    return _once(("limiter", nch, bool(true_peak), float(ceiling), names), make)


def limiter_bad(got, exp, nch, ceiling, names=NAMES):
    """the labels (pattern@g=gain) of the streams whose samples (bit patterns, a NaN against a NaN) or statistics differ"""
    import limiter_lib as LM
    labels = limiter_streams(nch, ceiling, names)[2]
    return [labels[i] for i in LM.bad_streams(got[0], got[1], *exp) if ("limiter", labels[i].split("@")[0]) not in EXCEPTIONS]


TONES_SPLIT = (2, 1, 3)


def tones_modes(nch):
    """(gated, shared) of the runs: sharing is a stereo tool; one mono run shows that the flag changes nothing there"""
    return ((False, False), (True, False), (False, True), (True, True)) if nch == 2 else ((False, False), (True, False), (False, True))


def _tones_writer(lib_path):
    """the frame writer of at3p_gha_lib.pipeline that prices the block (at3phip_write_frames_tonal, pinned to the reference by
    tests/test_at3p_tonal_*), one stream at a time"""
    from atracdenc_amd.binding import At3pHip

    def write(specs, recs):
        one = At3pHip(n_streams=1, max_frames=specs.shape[0], channels=specs.shape[1], lib_path=lib_path)
        try:
            return one.write_frames(specs[None], None, recs[None])[0]
        finally:
            one.close()
    return write


def tones_run(lib_path, nch, gated, shared, names=NAMES, split=None):
    """(records [S, 6], residuals [S, 6, nch, 16, 128], frames [S, 6, 2048]) of one context over at3p_batch(nch): analyse_tones on
    its own pqf(), then after a reset encode_frames_tonal, both fed whole or as `split`"""
    from atracdenc_amd.binding import AT3P_TONAL_BLOCK_DTYPE, At3pHip, _tone_flags
    pcm = at3p_batch(nch, names)
    S, nf = pcm.shape[:2]
    fl = _tone_flags(gated, shared)
    enc = At3pHip(n_streams=S, max_frames=nf, channels=nch, lib_path=lib_path)
    try:
        bands = enc.pqf(pcm)
        recs, resid, frames, at = [], [], [], 0
        for k in (split or (nf,)):
            piece = np.ascontiguousarray(bands[:, at:at + k])
            b = _sent((S, k, AT3P_TONAL_BLOCK_DTYPE.itemsize), np.uint8)
            r = _sent(piece.shape, np.float32)
            enc.analyse_tones_ptr(piece.ctypes.data, k, b.ctypes.data, r.ctypes.data, fl)
            recs.append(b.view(AT3P_TONAL_BLOCK_DTYPE).reshape(S, k))
            resid.append(r)
            at += k
        enc.reset()
        at = 0
        for k in (split or (nf,)):
            piece = np.ascontiguousarray(pcm[:, at:at + k])
            out = _sent((S, k, 2048), np.uint8)
            enc.encode_frames_tonal_ptr(piece.ctypes.data, k, out.ctypes.data, fl)
            frames.append(out)
            at += k
    finally:
        enc.close()
    return np.concatenate(recs, axis=1), np.concatenate(resid, axis=1), np.concatenate(frames, axis=1)


def tones_analysis(nch, gated, shared, names=NAMES):
    """(records [S, 6], residuals [S, 6, nch, 16, 128]) of tests/host/at3p_gha_cpu.c on the oracle's subbands, each stream alone"""
    import at3p_gha_lib as G

    def make():
        res = [G.CpuToneAnalyser(nch, gated, shared).analyse(G.pqf_bands(pcm)) for pcm in at3p_batch(nch, names)]
        return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])
    return _once(("tones", nch, bool(gated), bool(shared), names), make)


def tones_expect(lib_path, nch, gated, shared, names=NAMES):
    """(records, residuals, frames [S, 6, 2048]): tones_analysis(), and the frames at3p_gha_lib.pipeline builds from them (the
    division by 32768 / 1.122018, the oracle's MDCT and writer, the block spliced in), each stream alone. Where a block does not
    fit beside the oracle's quant units (stereo e15: 48 waves at the largest AmpSf), the stream's frames come from the writer of
    `lib_path`, which prices the block."""
    import at3p_gha_lib as G

    def make():
        recs, resid = tones_analysis(nch, gated, shared, names)
        frames = []
        for i in range(len(names)):
            with np.errstate(all="ignore"):
                specs = G.residual_specs(resid[i])
            wrecs, out = G.writer_records(recs[i]), []
            for fr, rec in zip(G.at3p_write_frames(specs), wrecs):
                b = G.block_dict(rec, nch)
                out.append(fr if b is None else G.splice_tonal(fr, G.tonal_bits(nch, b)))
            priced = any(fr is None for fr in out)
            assert not priced or (nch == 2 and names[i] == "e15"), (names[i], nch)
            frames.append(_tones_writer(lib_path)(specs, wrecs) if priced else np.stack(out))
        return recs, resid, np.stack(frames)
    return _once(("tones frames", lib_path, nch, bool(gated), bool(shared), names), make)


def tones_bad(got, exp, names=NAMES):
    """{"records" | "residuals" | "frames": the names of the streams that differ from the restatement of that stream alone}:
    records and frames byte for byte, residuals by floats_match"""
    live = [(i, n) for i, n in enumerate(names) if ("tones", n) not in EXCEPTIONS]
    return {"records": [n for i, n in live if got[0][i].tobytes() != exp[0][i].tobytes()],
            "residuals": [n for i, n in live if floats_match(got[1][i], exp[1][i]).any()],
            "frames": [n for i, n in live if not np.array_equal(got[2][i], exp[2][i])]}


# ---- the real reference build on the patterns, in a child process ----------------------------------------------------------
# (patterns for which the reference itself crashed or gave two different results would be listed here with what was seen,
# and in EXCEPTIONS: std::sort with NaN keys is outside its contract. None did.)
REF_UNDEFINED = {}
REF_AT3 = ((132300, 0, 0), (132300, 1, 1), (66150, 0, 0), (66150, 1, 1))
REF_AT1 = (("auto", 2), ("short", 2), ("auto", 1))


def ref_child(name, out_path):
    """the reference's encodes of one pattern, each made twice, into an .npz (run as `python float_domain_lib.py NAME OUT`)"""
    from at3_testlib import at1_ref_encode, ref
    r, out = ref(), {}
    pcm = stream(name)
    for br, ng, nt in REF_AT3:
        for k in range(2):
            out[f"at3_{br}_{ng}{nt}_{k}"] = r.encode(pcm, br, ng, nt)[0]
    for mode, nch in REF_AT1:
        blocks = at1_batch(nch, (name,))[0]
        for k in range(2):
            out[f"at1_{mode}_{nch}_{k}"] = at1_ref_encode(blocks, mode)
    np.savez(out_path, **out)


if __name__ == "__main__":
    import sys
    ref_child(sys.argv[1], sys.argv[2])
