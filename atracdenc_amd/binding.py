"""ctypes binding of include/at3hip.h (the same stub a maintainer would write for any FFI)."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libat3hip.so")
CSRC = os.path.join(HERE, "csrc")

AT3HIP_PCM_ON_DEVICE = 1
AT3HIP_OUT_ON_DEVICE = 2
AT3HIP_ASYNC = 4
OPT_RUNS, OPT_LITERAL_FORMS, OPT_QUANT_TAP, OPT_GAIN_FORM, OPT_GAIN_WGS_PER_CU, OPT_CHAIN, OPT_TIMING_EVERY = 1, 2, 3, 4, 5, 6, 7
OPT_FLATNESS_LITERAL = OPT_LITERAL_FORMS           # (former name, same number)
GAIN_FORM_TWO_WAVES, GAIN_FORM_ONE_WAVE = 0, 1
AT3HIP_VERSION = (1 << 16) | 6                     # include/at3hip.h this stub mirrors: load_library refuses an older library
TAP_SPECTRA, TAP_CURVES, TAP_ENERGY_SCALE, TAP_PSY, TAP_LOUDNESS, TAP_QUANT, TAP_CLOCK, TAP_GAIN_ANALYSIS = 1, 2, 3, 4, 5, 6, 7, 8
LP2 = 132300
LP4 = 66150


class At3HipError(RuntimeError):
    pass


class Config(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("bitrate", "channels", "no_gain_control", "no_tonal", "bfu_idx_const",
                                               "n_streams", "max_blocks", "device_id")]


class Counters(ctypes.Structure):
    _fields_ = [("scale_overflow", ctypes.c_uint64), ("clipped_values", ctypes.c_uint64)]


class Timings(ctypes.Structure):
    _fields_ = [(n, ctypes.c_float) for n in ("total_ms", "qmf_ms", "gain_ms", "curve_ms", "qmf_mdct_ms", "psy_ms",
                                               "alloc_ms")] + [("qmf_mdct_launches", ctypes.c_int32)]


AT3HIP_DECODE_S16 = 8
AT3HIP_RESAMPLE_OUT_S16 = 8                        # include/at3hip_resample.h: 16-bit output of the resampler
AT1HIP_DECODE_S16 = 8                              # include/at1hip.h
AT3PHIP_DECODE_S16 = 8                             # include/at3phip.h
AT3PHIP_FRAME_BYTES = 2048                         # the default frame size
AT3PHIP_MIN_FRAME_BYTES_MONO, AT3PHIP_MIN_FRAME_BYTES_STEREO = 176, 224   # the smallest admissible sizes (FRAME SIZE)
AT3PHIP_DECODE_TONES = 16
AT3PHIP_DECODE_SPARSE = 32   # at3phip_decode: word length 0 inside the coded range (include/at3phip.h, SPARSE WORD LENGTHS)
AT3PHIP_ALLOC_SPARSE = 256   # the frame-writing calls, with AT3PHIP_ALLOC_ADAPTIVE: a unit inside the coded range may keep word length 0
AT3PHIP_ALLOC_RD = 512       # the frame-writing calls, with both of the above: word lengths chosen by rate and distortion
AT3PHIP_ALLOC_PSY = 1024     # the frame-writing calls, with all three of the above: lambda shifted per unit by its masking threshold
AT3PHIP_DECODER_TABLES_BYTES = 67328
AT3PHIP_DECODER_TONE_TABLES_BYTES = 9504


class At1Config(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("channels", "window_auto", "window_mask", "bfu_idx_const", "n_streams", "max_blocks",
                                              "device_id")]


class At3pConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("channels", "n_streams", "max_frames", "device_id")]


class At1DecoderConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("channels", "n_streams", "max_frames", "device_id")]


class At1DecoderCounters(ctypes.Structure):
    _fields_ = [("bad_block_size", ctypes.c_uint64), ("read_past_end", ctypes.c_uint64)]


class At3DecoderConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("n_streams", "frame_size", "joint_stereo", "max_frames", "device_id")]


AT3_DECODER_REASONS = ("bad_id", "unsupported_js", "read_past_end", "tonal_past_end", "bad_tonal_mode", "bad_tonal_quant")


class At3DecoderCounters(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in AT3_DECODER_REASONS]


class At3pDecoderConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("channels", "n_streams", "max_frames", "device_id")]


AT3P_DECODER_REASONS = ("bad_header", "unsupported_syntax", "tonal_present", "bad_code", "read_past_end", "no_terminator")


class At3pDecoderCounters(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in AT3P_DECODER_REASONS]


class ResamplerConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("in_rate", "out_rate", "channels", "n_streams", "max_in", "device_id")]


class LoudnessConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("channels", "n_streams", "max_in", "max_hops", "true_peak", "device_id")]


class LoudnessResult(ctypes.Structure):
    _fields_ = [("integrated", ctypes.c_double), ("momentary_max", ctypes.c_double), ("short_term_max", ctypes.c_double),
                ("sample_peak", ctypes.c_float * 2), ("true_peak", ctypes.c_float * 2), ("n_samples", ctypes.c_int64),
                ("n_hops", ctypes.c_int32), ("n_blocks_kept", ctypes.c_int32)]

    def as_dict(self):
        """plain Python values; sample_peak / true_peak as numpy float32 [2]"""
        d = {n: getattr(self, n) for n in ("integrated", "momentary_max", "short_term_max", "n_samples", "n_hops", "n_blocks_kept")}
        d["sample_peak"] = np.array(self.sample_peak[:], np.float32)
        d["true_peak"] = np.array(self.true_peak[:], np.float32)
        return d


LOUDNESS_HOP = 4410


class LimitStats(ctypes.Structure):
    """at3hip_limit_stats: min_sum / LIMIT_FULL is the smallest smoothed gain of the run, n_limited of n_out outputs were reduced"""
    _fields_ = [("min_sum", ctypes.c_int64), ("n_limited", ctypes.c_int64), ("n_out", ctypes.c_int64)]


LIMIT_LOOKAHEAD, LIMIT_HOLD = 220, 2205
LIMIT_FULL = (LIMIT_LOOKAHEAD + 1) << 30
AT3HIP_LIMIT_TRUE_PEAK = 1


class At1Timings(ctypes.Structure):
    _fields_ = [(n, ctypes.c_float) for n in ("total_ms", "front_ms", "scan_ms", "pack_ms")]


_RC, _VP, _I32, _U32, _SZ, _STR = ctypes.c_int, ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32, ctypes.c_size_t, ctypes.c_char_p
_P = ctypes.POINTER
_I32P, _F32P, _RESP = _P(_I32), _P(ctypes.c_float), _P(LoudnessResult)
# name -> (restype, argtypes) of every exported function: load_library applies it, the three symbol lists are its names
PROTOTYPES = {
    # include/at3hip.h: the ATRAC3 encoder
    "at3hip_version": (_U32, []), "at3hip_device_numa_node": (_RC, [_I32]),
    "at3hip_create": (_RC, [_P(Config), _P(_VP)]), "at3hip_destroy": (None, [_VP]), "at3hip_last_error": (_STR, [_VP]),
    "at3hip_reset": (_RC, [_VP]), "at3hip_sync": (_RC, [_VP]), "at3hip_set_stream": (_RC, [_VP, _VP]),
    "at3hip_frame_size": (_RC, [_VP]), "at3hip_joint_stereo": (_RC, [_VP]), "at3hip_set_option": (_RC, [_VP, _I32, _I32]),
    "at3hip_encode": (_RC, [_VP, _VP, _I32, _VP, _I32P, _U32]), "at3hip_encode_s16": (_RC, [_VP, _VP, _I32, _VP, _I32P, _U32]),
    "at3hip_wait_input": (_RC, [_VP, _I32]), "at3hip_wait_frames": (_RC, [_VP, _I32]),
    "at3hip_mdct": (_RC, [_VP, _VP, _VP, _VP, _VP, _VP, _I32, _U32]),
    "at3hip_mdct_levels": (_RC, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _I32, _U32]),
    "at3hip_gain_energy_scale": (_RC, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I32, _U32]),
    "at3hip_qmf_mdct": (_RC, [_VP, _VP, _I32, _VP, _U32]), "at3hip_read_tap": (_RC, [_VP, _I32, _VP, _SZ]),
    "at3hip_get_timings": (_RC, [_VP, _P(Timings)]), "at3hip_get_timings_ago": (_RC, [_VP, _I32, _P(Timings)]),
    "at3hip_get_counters": (_RC, [_VP, _P(Counters), _I32]), "at3hip_host_tables": (_RC, [_VP, _SZ]),
    "at3hip_host_alloc": (_RC, [_VP, _SZ, _P(_VP)]), "at3hip_host_free": (_RC, [_VP, _VP]),
    # include/at3hip.h: the ATRAC3 decoder
    "at3hip_decoder_create": (_RC, [_P(At3DecoderConfig), _P(_VP)]), "at3hip_decoder_destroy": (None, [_VP]),
    "at3hip_decoder_last_error": (_STR, [_VP]), "at3hip_decoder_reset": (_RC, [_VP]), "at3hip_decoder_sync": (_RC, [_VP]),
    "at3hip_decoder_set_stream": (_RC, [_VP, _VP]), "at3hip_decode": (_RC, [_VP, _VP, _I32, _VP, _U32]),
    "at3hip_decoder_get_counters": (_RC, [_VP, _P(At3DecoderCounters), _I32]),
    # include/at3hip_resample.h (listed in at3hip.h's version notes)
    "at3hip_resampler_create": (_RC, [_P(ResamplerConfig), _P(_VP)]), "at3hip_resampler_destroy": (None, [_VP]),
    "at3hip_resampler_last_error": (_STR, [_VP]), "at3hip_resampler_reset": (_RC, [_VP]), "at3hip_resampler_sync": (_RC, [_VP]),
    "at3hip_resampler_set_stream": (_RC, [_VP, _VP]), "at3hip_resampler_max_out": (_I32, [_VP]),
    "at3hip_resampler_process": (_RC, [_VP, _VP, _I32, _VP, _I32P, _U32]),
    "at3hip_resampler_process_s16": (_RC, [_VP, _VP, _I32, _VP, _I32P, _U32]),
    "at3hip_resampler_flush": (_RC, [_VP, _VP, _I32P, _U32]),
    "at3hip_resampler_shape": (_RC, [_I32, _I32, _I32P, _I32P, _I32P]), "at3hip_resampler_host_tables": (_RC, [_I32, _I32, _VP, _SZ]),
    # include/at3hip_loudness.h (listed in at3hip.h's version notes)
    "at3hip_loudness_create": (_RC, [_P(LoudnessConfig), _P(_VP)]), "at3hip_loudness_destroy": (None, [_VP]),
    "at3hip_loudness_last_error": (_STR, [_VP]), "at3hip_loudness_reset": (_RC, [_VP]), "at3hip_loudness_sync": (_RC, [_VP]),
    "at3hip_loudness_set_stream": (_RC, [_VP, _VP]),
    "at3hip_loudness_process": (_RC, [_VP, _VP, _I32, _U32]), "at3hip_loudness_process_s16": (_RC, [_VP, _VP, _I32, _U32]),
    "at3hip_loudness_apply": (_RC, [_VP, _VP, _I32, _VP, _VP, _U32]), "at3hip_loudness_apply_s16": (_RC, [_VP, _VP, _I32, _VP, _VP, _U32]),
    "at3hip_loudness_finish": (_RC, [_VP, _RESP]), "at3hip_loudness_read_hops": (_RC, [_VP, _I32, _VP, _SZ]),
    "at3hip_loudness_gate": (_RC, [_VP, _I32, _I32, _RESP]), "at3hip_loudness_gain": (_RC, [_RESP, ctypes.c_double, ctypes.c_double, _F32P]),
    "at3hip_loudness_limit_start": (_RC, [_VP, _VP, ctypes.c_float, _U32]), "at3hip_loudness_limit_delay": (_I32, [_U32]),
    "at3hip_loudness_limit": (_RC, [_VP, _VP, _I32, _VP, _I32P, _U32]), "at3hip_loudness_limit_s16": (_RC, [_VP, _VP, _I32, _VP, _I32P, _U32]),
    "at3hip_loudness_limit_flush": (_RC, [_VP, _VP, _I32P, _U32]), "at3hip_loudness_limit_stats": (_RC, [_VP, _P(LimitStats)]),
    # include/at1hip.h: the ATRAC1 encoder
    "at1hip_create": (_RC, [_P(At1Config), _P(_VP)]), "at1hip_destroy": (None, [_VP]), "at1hip_last_error": (_STR, [_VP]),
    "at1hip_reset": (_RC, [_VP]), "at1hip_sync": (_RC, [_VP]),
    "at1hip_encode": (_RC, [_VP, _VP, _I32, _VP, _U32]), "at1hip_encode_short": (_RC, [_VP, _VP, _I32, _VP, _U32]),
    "at1hip_get_timings": (_RC, [_VP, _P(At1Timings)]), "at1hip_read_tap": (_RC, [_VP, _I32, _VP, _SZ]),
    "at1hip_host_tables": (_RC, [_VP, _SZ]),
    # include/at1hip.h: the ATRAC1 decoder
    "at1hip_decoder_create": (_RC, [_P(At1DecoderConfig), _P(_VP)]), "at1hip_decoder_destroy": (None, [_VP]),
    "at1hip_decoder_last_error": (_STR, [_VP]), "at1hip_decoder_reset": (_RC, [_VP]), "at1hip_decoder_sync": (_RC, [_VP]),
    "at1hip_decoder_set_stream": (_RC, [_VP, _VP]), "at1hip_decode": (_RC, [_VP, _VP, _I32, _VP, _U32]),
    "at1hip_decoder_get_counters": (_RC, [_VP, _P(At1DecoderCounters), _I32]),
    # include/at3phip.h: the ATRAC3plus encoder
    "at3phip_create": (_RC, [_P(At3pConfig), _P(_VP)]), "at3phip_destroy": (None, [_VP]), "at3phip_last_error": (_STR, [_VP]),
    "at3phip_reset": (_RC, [_VP]), "at3phip_sync": (_RC, [_VP]),
    "at3phip_pqf_analyse": (_RC, [_VP, _VP, _I32, _VP, _U32]), "at3phip_mdct": (_RC, [_VP, _VP, _I32, _VP, _VP, _U32]),
    "at3phip_pqf_mdct": (_RC, [_VP, _VP, _I32, _VP, _VP, _VP, _U32]), "at3phip_write_frames": (_RC, [_VP, _VP, _I32, _VP, _VP, _U32]),
    "at3phip_write_frames_tonal": (_RC, [_VP, _VP, _I32, _VP, _VP, _VP, _U32]),
    "at3phip_encode_frames": (_RC, [_VP, _VP, _I32, _VP, _U32]), "at3phip_encode_frames_short": (_RC, [_VP, _VP, _I32, _VP, _U32]),
    "at3phip_analyse_tones": (_RC, [_VP, _VP, _I32, _VP, _VP, _U32]),
    "at3phip_encode_frames_tonal": (_RC, [_VP, _VP, _I32, _VP, _U32]), "at3phip_encode_frames_tonal_short": (_RC, [_VP, _VP, _I32, _VP, _U32]),
    "at3phip_get_timings": (_RC, [_VP, _F32P, _F32P]), "at3phip_get_write_timing": (_RC, [_VP, _F32P]),
    "at3phip_host_tables": (_RC, [_VP, _SZ]), "at3phip_host_write_tables": (_RC, [_VP, _SZ]),
    "at3phip_host_tone_find_tables": (_RC, [_VP, _SZ]), "at3phip_host_tone_gates": (_RC, [_VP, _I32, _I32, _VP]),
    "at3phip_host_tone_flags": (_U32, []), "at3phip_host_allocate": (_RC, [_VP, _VP, _I32, _I32, _VP, _VP, _VP, _VP]),
    "at3phip_host_allocate_sized": (_RC, [_VP, _VP, _I32, _I32, _I32, _VP, _VP, _VP, _VP]),
    "at3phip_host_allocate_sparse": (_RC, [_VP, _VP, _I32, _I32, _I32, _VP, _VP, _VP, _VP]),
    "at3phip_host_allocate_rd": (_RC, [_VP, _VP, _VP, _I32, _I32, _I32, _VP, _VP, _VP, _VP, _VP]),
    "at3phip_host_allocate_psy": (_RC, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _VP, _VP, _VP, _VP, _VP, _VP]),
    "at3phip_set_frame_bytes": (_RC, [_VP, _I32]), "at3phip_get_frame_bytes": (_RC, [_VP, _I32P]),
    "at3phip_decoder_set_frame_bytes": (_RC, [_VP, _I32]), "at3phip_decoder_get_frame_bytes": (_RC, [_VP, _I32P]),
    # include/at3phip.h: the ATRAC3plus decoder
    "at3phip_decoder_create": (_RC, [_P(At3pDecoderConfig), _P(_VP)]), "at3phip_decoder_destroy": (None, [_VP]),
    "at3phip_decoder_last_error": (_STR, [_VP]), "at3phip_decoder_reset": (_RC, [_VP]), "at3phip_decoder_sync": (_RC, [_VP]),
    "at3phip_decoder_set_stream": (_RC, [_VP, _VP]), "at3phip_decode": (_RC, [_VP, _VP, _I32, _VP, _U32]),
    "at3phip_decoder_get_counters": (_RC, [_VP, _P(At3pDecoderCounters), _I32]),
    "at3phip_decoder_host_tables": (_RC, [_VP, _SZ]), "at3phip_decoder_host_tone_tables": (_RC, [_VP, _SZ]),
}
SYMBOLS = [n for n in PROTOTYPES if n.startswith("at3hip_")]
AT1_SYMBOLS = [n for n in PROTOTYPES if n.startswith("at1hip_")]
AT3P_SYMBOLS = [n for n in PROTOTYPES if n.startswith("at3phip_")]


def build_library(verbose=False):
    """Compile libat3hip.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "-fvisibility=hidden", "-fPIC", "-shared",
           "-Wl,--version-script=" + os.path.join(CSRC, "exports.map"), "-o", LIB_PATH, os.path.join(CSRC, "at3hip.hip"), os.path.join(CSRC, "at1hip.hip"), os.path.join(CSRC, "at3phip.hip"),
           os.path.join(CSRC, "at3p_alloc.hip"), os.path.join(CSRC, "at3p_sparse.hip"), os.path.join(CSRC, "at3p_rd.hip"), os.path.join(CSRC, "at3p_psy.hip"), os.path.join(CSRC, "resample.hip"), os.path.join(CSRC, "loudness.hip"), os.path.join(CSRC, "at3_tables.cpp")]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return LIB_PATH


_lib_cache = {}


def load_library(path=None):
    path = path or os.environ.get("AT3HIP_LIB") or LIB_PATH
    if path in _lib_cache:
        return _lib_cache[path]
    # PyTorch wheels bundle their own HIP runtime; when torch shares the process (bench.py, tests) it has
    # to be loaded first so that libat3hip.so binds to the same runtime instance instead of a second copy.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    if not os.path.exists(path):
        raise At3HipError(f"{path} not found: build it with atracdenc_amd.build_library() / __graft_entry__.build(); "
                          "there is no CPU fallback")
    lib = ctypes.CDLL(path)
    lib.at3hip_version.restype = ctypes.c_uint32
    have = lib.at3hip_version()
    # same major number, and every entry point / option / wait depth this stub relies on (at3hip.h lists them per minor number)
    if have >> 16 != AT3HIP_VERSION >> 16 or have < AT3HIP_VERSION:
        raise At3HipError(f"{path} implements at3hip ABI {have >> 16}.{have & 0xffff}, this binding needs {AT3HIP_VERSION >> 16}.{AT3HIP_VERSION & 0xffff}: rebuild it")
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name, None)   # what was added under ABI 1.6 is detected by symbol (at3hip.h's version list): see _need
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
    _lib_cache[path] = lib
    return lib


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _need(lib, name):
    """the function `name` of lib; a library that predates it is an error (nothing is emulated on the host instead)"""
    fn = getattr(lib, name, None)
    if fn is None:
        raise At3HipError(f"libat3hip.so predates {name}: rebuild it")
    return fn


def _lib_call(lib_path, name, *args, why=""):
    """`name`(*args) of the library for a function that takes no context, raising At3HipError on failure."""
    rc = _need(load_library(lib_path), name)(*args)
    if rc != 0:
        raise At3HipError(f"{name} failed ({rc}){why}")


def _host_tables(lib_path, name, out, *args):
    """fills `out` with the table block that `name` builds on this host (no GPU involved)"""
    _lib_call(lib_path, name, *args, _vp(out), out.nbytes, why=f": the table block is {out.nbytes} bytes here")
    return out


def _device_flags(asynchronous):
    return AT3HIP_PCM_ON_DEVICE | AT3HIP_OUT_ON_DEVICE | (AT3HIP_ASYNC if asynchronous else 0)


class _Context:
    """One C-ABI context of `lib`: <_PREFIX>_create / _destroy / _last_error / _reset / _sync. Every call into the library
    that takes the context goes through _call (a status) or _value (a plain number)."""

    _PREFIX = ""

    def _create(self, cfg, hint):
        self.cfg = cfg
        self.ctx = ctypes.c_void_p()
        rc = _need(self.lib, self._PREFIX + "_create")(ctypes.byref(cfg), ctypes.byref(self.ctx))
        if rc != 0:
            self.ctx = None
            raise At3HipError(f"{self._PREFIX}_create failed with {rc} ({hint})")

    def close(self):
        if getattr(self, "ctx", None):
            getattr(self.lib, self._PREFIX + "_destroy")(self.ctx)
            self.ctx = None

    def __del__(self):
        self.close()

    def _check(self, rc, what):
        if rc != 0:
            raise At3HipError(f"{what} failed ({rc}): {getattr(self.lib, self._PREFIX + '_last_error')(self.ctx).decode()}")

    def _call(self, name, *args, prefix=None):
        """<_PREFIX>_<name>(ctx, *args), raising At3HipError with that function's name on failure (prefix: instead of _PREFIX)."""
        fn = f"{prefix or self._PREFIX}_{name}"
        self._check(_need(self.lib, fn)(self.ctx, *args), fn)

    def _value(self, name):
        """<_PREFIX>_<name>(ctx) of a function that returns a number, not a status."""
        return _need(self.lib, f"{self._PREFIX}_{name}")(self.ctx)

    def reset(self):
        self._call("reset")

    def sync(self):
        self._call("sync")

    def _order_behind_torch(self, device, ordered):
        """Queues the next call on torch's current stream of `device` (ordered), or on the context's own stream. Torch's
        default stream is the null stream, whose handle (0) means "the context's own stream" to <_PREFIX>_set_stream;
        the context's stream is non-blocking: wait for what torch queued there instead."""
        stream = None
        if ordered:
            import torch
            cur = torch.cuda.current_stream(device)
            stream = cur.cuda_stream or None
            if stream is None:
                cur.synchronize()
        self._call("set_stream", ctypes.c_void_p(stream))


class _Decoder(_Context):
    """A batched decoder: <_CODEC>_decode and the <_CODEC>_decoder_* lifecycle, with counters named by _COUNTERS' fields.
    A subclass gives _shapes(); its decode / decode_device are _decode / _decode_device under its own argument names."""

    _CODEC = ""        # <_CODEC>_decode; the lifecycle functions are <_PREFIX>_*
    _COUNTERS = None   # the ctypes structure <_PREFIX>_get_counters fills

    def _shapes(self):
        """(shape of one frame's bytes, shape of one frame's samples): what follows [n_streams, n_frames]"""
        raise NotImplementedError

    def decode_ptr(self, src_ptr, n_frames, out_ptr, flags):
        """Raw pointers and <_CODEC>_decode flags (benchmarks)."""
        self._call("decode", ctypes.c_void_p(src_ptr), int(n_frames), ctypes.c_void_p(out_ptr), int(flags), prefix=self._CODEC)

    def _decode(self, frames, s16, flags=0):
        """host uint8 [n_streams, n_frames, *frame bytes] -> float32 (int16 with s16) [n_streams, n_frames, *frame samples];
        the three <_CODEC>_DECODE_S16 flags are one number"""
        src, dst = self._shapes()
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        assert frames.ndim == 2 + len(src) and frames.shape[0] == self.n_streams and frames.shape[2:] == src, frames.shape
        n = frames.shape[1]
        out = np.zeros((self.n_streams, n) + dst, dtype=np.int16 if s16 else np.float32)
        self.decode_ptr(frames.ctypes.data, n, out.ctypes.data, (AT3HIP_DECODE_S16 if s16 else 0) | flags)
        return out

    def _decode_device(self, frames, out, asynchronous, ordered, flags=0):
        """torch tensors of the shapes of _decode on this decoder's device"""
        import torch
        src, dst = self._shapes()
        assert frames.dtype == torch.uint8 and frames.is_contiguous() and out.is_contiguous()
        assert out.dtype in (torch.float32, torch.int16)
        n = frames.shape[1]
        assert tuple(frames.shape) == (self.n_streams, n) + src, tuple(frames.shape)
        assert tuple(out.shape) == (self.n_streams, n) + dst, tuple(out.shape)
        flags |= _device_flags(asynchronous) | (AT3HIP_DECODE_S16 if out.dtype == torch.int16 else 0)
        self._order_behind_torch(frames.device, ordered)
        self.decode_ptr(frames.data_ptr(), n, out.data_ptr(), flags)

    def counters(self, reset=False):
        c = self._COUNTERS()
        self._call("get_counters", ctypes.byref(c), int(bool(reset)))
        return {n: int(getattr(c, n)) for n, _ in self._COUNTERS._fields_}


def _curves(n_points, level, loc):
    """the three optional gain-curve arrays as int32 (kept alive by the caller) and their pointers"""
    if n_points is None:
        return (), (None, None, None)
    arrays = tuple(np.ascontiguousarray(a, dtype=np.int32) for a in (n_points, level, loc))
    return arrays, tuple(_vp(a) for a in arrays)


class At3Hip(_Context):
    """n_streams TAtrac3Encoder objects encoded side by side on one GPU."""

    _PREFIX = "at3hip"

    def __init__(self, n_streams=1, max_blocks=64, bitrate=LP2, no_gain=False, no_tonal=False, bfu_idx_const=0,
                 device_id=0, lib_path=None, channels=2):
        self.lib = load_library(lib_path)
        self.channels = int(channels)
        self._create(Config(int(bitrate), int(channels), int(no_gain), int(no_tonal), int(bfu_idx_const), int(n_streams),
                            int(max_blocks), int(device_id)), "no usable MI355X / HIP runtime?")
        self.n_streams = n_streams
        self.frame_size = self._value("frame_size")
        self.joint_stereo = bool(self._value("joint_stereo"))

    def encode_ptr(self, pcm_ptr, n_blocks, out_ptr, flags):
        """Raw pointers (float32 PCM) and at3hip_encode flags; returns frames per stream."""
        nf = ctypes.c_int32()
        self._call("encode", ctypes.c_void_p(pcm_ptr), int(n_blocks), ctypes.c_void_p(out_ptr), ctypes.byref(nf), int(flags))
        return nf.value

    def encode_s16_ptr(self, pcm_ptr, n_blocks, out_ptr, flags):
        """Raw pointers (int16 PCM) and at3hip_encode_s16 flags; returns frames per stream."""
        nf = ctypes.c_int32()
        self._call("encode_s16", ctypes.c_void_p(pcm_ptr), int(n_blocks), ctypes.c_void_p(out_ptr), ctypes.byref(nf), int(flags))
        return nf.value

    def _encode_host(self, pcm, dtype, raw):
        pcm = np.ascontiguousarray(pcm, dtype=dtype)
        assert pcm.ndim == 4 and pcm.shape[0] == self.n_streams and pcm.shape[2:] == (1024, self.channels), pcm.shape
        nb = pcm.shape[1]
        out = np.zeros((self.n_streams, nb, self.frame_size), dtype=np.uint8)
        n = raw(pcm.ctypes.data, nb, out.ctypes.data, 0)
        return np.ascontiguousarray(out.reshape(-1)[: self.n_streams * n * self.frame_size].reshape(
            self.n_streams, n, self.frame_size))

    def encode(self, pcm):
        """pcm float32 [n_streams, n_blocks, 1024, channels] (host) -> uint8 [n_streams, n_frames, frame_size]."""
        return self._encode_host(pcm, np.float32, self.encode_ptr)

    def encode_s16(self, pcm):
        """pcm int16 [n_streams, n_blocks, 1024, channels] (host) -> uint8 [n_streams, n_frames, frame_size] (at3hip_encode_s16)."""
        return self._encode_host(pcm, np.int16, self.encode_s16_ptr)

    def encode_device(self, pcm_ptr, n_blocks, out_ptr, asynchronous=False):
        """Device-resident PCM/out (raw pointers, e.g. torch tensor .data_ptr()). Returns frames per stream.
        asynchronous=True only queues the work (AT3HIP_ASYNC): call sync() before the frames are read."""
        return self.encode_ptr(pcm_ptr, n_blocks, out_ptr, _device_flags(asynchronous))

    def encode_device_s16(self, pcm_ptr, n_blocks, out_ptr, asynchronous=False):
        """Device-resident int16 PCM / out (raw pointers). Returns frames per stream."""
        return self.encode_s16_ptr(pcm_ptr, n_blocks, out_ptr, _device_flags(asynchronous))

    PSY_DTYPE = np.dtype([("loud_ch", "<f4"), ("n_tonal", "<i4"), ("sfi", "u1", 32), ("energy", "<f4", 32),
                          ("tonal", [("pos", "<u2"), ("bfu", "u1"), ("len", "u1"), ("sfi", "u1"), ("pad", "u1", 3),
                                     ("values", "<f4", 7), ("pad2", "u1", 4)], 24), ("flat", "<f4", 32)])
    QUANT_DTYPE = np.dtype([("err", "<f4", (7, 32)), ("cost", "<u4", (7, 32))])

    def read_tap(self, kind, dtype, shape):
        """Stage tap of the most recent encode call (AT3HIP_TAP_*), as a numpy array of `dtype` and `shape`."""
        out = np.zeros(shape, dtype=dtype)
        self._call("read_tap", int(kind), _vp(out), out.nbytes)
        return out

    def sclk_mhz(self):
        """Shader clock observed under the last call's rate loop (AT3HIP_TAP_CLOCK: s_memtime cycles against the 100 MHz
        s_memrealtime over the life of the allocation kernel's workgroup 0), or None before the first frames."""
        c = self.read_tap(TAP_CLOCK, np.uint64, (2,))
        return float(c[0]) / float(c[1]) * 100.0 if c[1] else None

    def counters(self, reset=False):
        """at3hip_get_counters: what TScaler::Scale would have printed since create / reset - {"scale_overflow", "clipped_values"}."""
        c = Counters()
        self._call("get_counters", ctypes.byref(c), int(bool(reset)))
        return {"scale_overflow": int(c.scale_overflow), "clipped_values": int(c.clipped_values)}

    def host_alloc(self, shape, dtype):
        """Page-locked host array (at3hip_host_alloc); free it with host_free(array) before close()."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = ctypes.c_void_p()
        self._call("host_alloc", n, ctypes.byref(p))
        buf = (ctypes.c_char * n).from_address(p.value)
        a = np.frombuffer(buf, dtype=dtype).reshape(shape)
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[a.ctypes.data] = p
        return a

    def host_free(self, a):
        self._call("host_free", self._pinned.pop(a.ctypes.data))

    def encode_host_async(self, pcm, out):
        """Queues one call on host arrays (pinned ones overlap copies and kernels); returns frames per stream. `out` is valid
        after wait_frames(ago) / sync(), `pcm` may be refilled after wait_input(ago)."""
        raw = self.encode_s16_ptr if pcm.dtype == np.int16 else self.encode_ptr
        return raw(pcm.ctypes.data, pcm.shape[1], out.ctypes.data, AT3HIP_ASYNC)

    def wait_input(self, ago=0):
        self._call("wait_input", int(ago))

    def wait_frames(self, ago=0):
        self._call("wait_frames", int(ago))

    def set_option(self, option, value):
        """AT3HIP_OPT_*: work partitioning / equivalent-form switches; results never change."""
        self._call("set_option", int(option), int(value))

    def set_stream(self, hip_stream):
        """Queue the front half on the caller's HIP stream (a hipStream_t handle, e.g. torch.cuda.Stream().cuda_stream);
        0 / None goes back to the context's own stream."""
        self._call("set_stream", ctypes.c_void_p(int(hip_stream) if hip_stream else None))

    def timings_ago(self, ago):
        t = Timings()
        self._call("get_timings_ago", int(ago), ctypes.byref(t))
        return {n: getattr(t, n) for n, _ in Timings._fields_}

    def qmf_mdct_device(self, pcm_ptr, n_blocks, specs_ptr):
        self._call("qmf_mdct", ctypes.c_void_p(pcm_ptr), n_blocks, ctypes.c_void_p(specs_ptr), _device_flags(False))

    def mdct(self, bands, n_points=None, level=None, loc=None, max_levels=False):
        """Batched TAtrac3MDCT::Mdct. bands float32 [n,4,512] -> (specs [n,1024], mutated bands[, max levels [n,4]])."""
        bands = np.ascontiguousarray(bands, dtype=np.float32).copy()
        n = bands.shape[0]
        specs = np.zeros((n, 1024), dtype=np.float32)
        keep, curves = _curves(n_points, level, loc)
        if max_levels:
            mx = np.zeros((n, 4), dtype=np.float32)
            self._call("mdct_levels", _vp(bands), _vp(specs), _vp(mx), *curves, n, 0)
            return specs, bands, mx
        self._call("mdct", _vp(bands), _vp(specs), *curves, n, 0)
        return specs, bands

    def gain_energy_scale(self, prev_overlap, cur_input, prev_scale, n_points=None, level=None, loc=None):
        """Batched TAtrac3MDCT::CalcGainEnergyScale. prev_overlap / cur_input float32 [n,256], prev_scale [n], optional
        n_points [n], level / loc [n,8] -> float32 [n,4] (PrevHalf, CurHalf, Frame, NextOverlapScale)."""
        prev_overlap = np.ascontiguousarray(prev_overlap, dtype=np.float32)
        cur_input = np.ascontiguousarray(cur_input, dtype=np.float32)
        prev_scale = np.ascontiguousarray(prev_scale, dtype=np.float32)
        n = prev_overlap.shape[0]
        out = np.zeros((n, 4), dtype=np.float32)
        keep, curves = _curves(n_points, level, loc)
        self._call("gain_energy_scale", _vp(prev_overlap), _vp(cur_input), *curves, _vp(prev_scale), _vp(out), n, 0)
        return out

    def timings(self):
        t = Timings()
        self._call("get_timings", ctypes.byref(t))
        return {n: getattr(t, n) for n, _ in Timings._fields_}


# atracdenc_amd/csrc/at3_tables.hpp, struct Tables (cpx = two float32)
AT3_TABLES_DTYPE = np.dtype([("qmf_win", "<f4", 48), ("scale", "<f4", 64), ("enc_win", "<f4", 256), ("gain_level", "<f4", 16),
                             ("gain_interp", "<f4", 32), ("mdct_sincos", "<f4", 256), ("planck", "<f4", 512), ("hpf_w", "<f4", 4),
                             ("loud_curve", "<f4", 1024), ("ath_bfu", "<f4", 32), ("tw128", "<f4", (128, 2)), ("tw256", "<f4", (256, 2)),
                             ("stw256", "<f4", (128, 2)), ("tw2048", "<f4", (2048, 2)), ("stw2048", "<f4", (1024, 2)),
                             ("log2f_tab", "<f8", (16, 2)), ("log2f_poly", "<f8", 4), ("gain_tw", "<f4", (27, 128, 2)),
                             ("ga1_twb", "<f4", (2, 15, 16, 2)), ("ga1_twc", "<f4", (8, 3, 64, 2)),
                             ("mdct_tab", "<f4", (18, 16, 4)), ("spec16_win", "<f4", (16, 16, 2)), ("spec16_tw", "<f4", (15, 16, 2)), ("spec16_stw", "<f4", (9, 16, 2)), ("log_c", "<f8", 18),
                             ("log_tab", "<f8", (128, 2)), ("exp_c", "<f8", 8), ("exp_tab", "<u8", (128, 2))])


def at3_host_tables(lib_path=None):
    """The ATRAC3 constant tables as the library builds them on this host (no GPU involved)."""
    return _host_tables(lib_path, "at3hip_host_tables", np.zeros((), dtype=AT3_TABLES_DTYPE))


AT1_TABLES_DTYPE = np.dtype([("qmf_win", "<f4", 48), ("scale", "<f4", 64), ("sine", "<f4", 32), ("sc512", "<f4", 256),
                             ("sc256", "<f4", 128), ("sc64", "<f4", 32), ("tw128", "<f4", 256), ("tw64", "<f4", 128),
                             ("tw16", "<f4", 32), ("loud", "<f4", 512), ("ath_bfu", "<f4", 52), ("fir", "<f4", 10),
                             ("fix_long", "<f4", 52), ("fix_short", "<f4", 52), ("logf", "<f8", 36)])
assert AT1_TABLES_DTYPE.itemsize == 6904


def at1_host_tables(lib_path=None):
    """The ATRAC1 constant tables as the library builds them on the host (no GPU involved)."""
    return _host_tables(lib_path, "at1hip_host_tables", np.zeros((), dtype=AT1_TABLES_DTYPE))


class At1Hip(_Context):
    """n_streams TAtrac1Encoder objects encoded side by side on one GPU (include/at1hip.h)."""

    _PREFIX = "at1hip"
    FRAME = 212
    TAP_SPECTRA, TAP_MASKS, TAP_LOUDNESS, TAP_TABLES = 1, 2, 3, 4

    def __init__(self, n_streams=1, max_blocks=64, channels=2, window_auto=True, window_mask=0, bfu_idx_const=0, device_id=0,
                 lib_path=None):
        self.lib = load_library(lib_path)
        self.channels, self.n_streams = int(channels), int(n_streams)
        self._create(At1Config(int(channels), int(bool(window_auto)), int(window_mask), int(bfu_idx_const), int(n_streams),
                               int(max_blocks), int(device_id)), "no usable MI355X / HIP runtime?")

    def encode_ptr(self, pcm_ptr, n_blocks, out_ptr, flags):
        """Raw pointers (float32 PCM) and at1hip_encode flags."""
        self._call("encode", ctypes.c_void_p(pcm_ptr), int(n_blocks), ctypes.c_void_p(out_ptr), int(flags))

    def encode_s16_ptr(self, pcm_ptr, n_blocks, out_ptr, flags):
        """Raw pointers (int16 PCM, 2-byte alignment is enough) and at1hip_encode_short flags."""
        self._call("encode_short", ctypes.c_void_p(pcm_ptr), int(n_blocks), ctypes.c_void_p(out_ptr), int(flags))

    def _encode_host(self, pcm, dtype, raw):
        pcm = np.ascontiguousarray(pcm, dtype=dtype)
        assert pcm.ndim == 4 and pcm.shape[0] == self.n_streams and pcm.shape[2:] == (512, self.channels), pcm.shape
        nb = pcm.shape[1]
        out = np.zeros((self.n_streams, nb, self.channels, self.FRAME), dtype=np.uint8)
        raw(pcm.ctypes.data, nb, out.ctypes.data, 0)
        return out

    def encode(self, pcm):
        """pcm float32 [n_streams, n_blocks, 512, channels] (host) -> uint8 [n_streams, n_blocks, channels, 212]."""
        return self._encode_host(pcm, np.float32, self.encode_ptr)

    def encode_s16(self, pcm):
        """pcm int16 [n_streams, n_blocks, 512, channels] (host) -> uint8 [n_streams, n_blocks, channels, 212]
        (at1hip_encode_short): the frames of encode() on pcm / 32768 as float32, bit for bit; the samples cross the bus as
        16-bit and are widened by the first kernel. Calls of both kinds may alternate."""
        return self._encode_host(pcm, np.int16, self.encode_s16_ptr)

    def encode_device(self, pcm_ptr, n_blocks, out_ptr, asynchronous=False):
        """Device-resident float32 PCM / frames (raw pointers). The context's stream is non-blocking (at3hip.h, DEVICE BUFFERS
        AND STREAMS): it waits for no other stream, so whatever produces the PCM must be complete before the call, and with
        asynchronous=True (AT3HIP_ASYNC) both buffers stay untouched until sync()."""
        self.encode_ptr(pcm_ptr, n_blocks, out_ptr, _device_flags(asynchronous))

    def encode_device_s16(self, pcm_ptr, n_blocks, out_ptr, asynchronous=False):
        """Device-resident int16 PCM / frames (raw pointers; the PCM needs only 2-byte alignment). Stream ordering and what
        stays untouched until sync() as in encode_device."""
        self.encode_s16_ptr(pcm_ptr, n_blocks, out_ptr, _device_flags(asynchronous))

    def read_tap(self, kind, dtype, shape):
        out = np.zeros(shape, dtype=dtype)
        self._call("read_tap", int(kind), _vp(out), out.nbytes)
        return out

    def timings(self):
        t = At1Timings()
        self._call("get_timings", ctypes.byref(t))
        return {n: getattr(t, n) for n, _ in At1Timings._fields_}


class At1HipDecoder(_Decoder):
    """n_streams TAtrac1Decoder objects decoded side by side on one GPU (include/at1hip.h, the decoder section)."""

    _CODEC, _PREFIX, _COUNTERS = "at1hip", "at1hip_decoder", At1DecoderCounters
    FRAME = 212

    def __init__(self, n_streams=1, max_frames=256, channels=2, device_id=0, lib_path=None):
        self.lib = load_library(lib_path)
        self.channels, self.n_streams, self.max_frames = int(channels), int(n_streams), int(max_frames)
        self._create(At1DecoderConfig(self.channels, self.n_streams, self.max_frames, int(device_id)),
                     "bad configuration, or no usable MI355X / HIP runtime")

    def _shapes(self):
        return (self.channels, self.FRAME), (512, self.channels)

    def decode(self, units, s16=False):
        """units uint8 [n_streams, n_frames, channels, 212] (host) -> float32 (int16 with s16) [n_streams, n_frames, 512, channels]."""
        return self._decode(units, s16)

    def decode_device(self, units, out, asynchronous=False, ordered=True):
        """Torch tensors on this decoder's device: units uint8 [n_streams, n, channels, 212] -> out float32 / int16 (s16 output)
        [n_streams, n, 512, channels]. By default the call is queued on torch's current stream, behind whatever filled `units`
        there (at1hip_decoder_set_stream; on torch's null default stream the call waits for it instead), and whatever torch queues
        there afterwards follows it (with asynchronous=True and the null stream: after sync()). ordered=False runs it on the
        decoder's own non-blocking stream: the caller must then make sure `units` is complete (the caller's race of
        at3hip.h's DEVICE BUFFERS AND STREAMS)."""
        self._decode_device(units, out, asynchronous, ordered)


class At3HipDecoder(_Decoder):
    """n_streams ATRAC3 streams of one container row decoded side by side on one GPU (include/at3hip.h, the decoder section)."""

    _CODEC, _PREFIX, _COUNTERS = "at3hip", "at3hip_decoder", At3DecoderCounters
    ROWS = {192: True, 272: True, 304: False, 384: False, 424: False, 512: False, 768: False, 1024: False}

    def __init__(self, n_streams=1, frame_size=384, joint_stereo=None, max_frames=256, device_id=0, lib_path=None):
        self.lib = load_library(lib_path)
        self.n_streams, self.frame_size, self.max_frames = int(n_streams), int(frame_size), int(max_frames)
        self.joint_stereo = bool(self.ROWS.get(self.frame_size, False) if joint_stereo is None else joint_stereo)
        self._create(At3DecoderConfig(self.n_streams, self.frame_size, int(self.joint_stereo), self.max_frames, int(device_id)),
                     "bad configuration, or no usable MI355X / HIP runtime")

    def _shapes(self):
        return (self.frame_size,), (1024, 2)

    def decode(self, frames, s16=False):
        """frames uint8 [n_streams, n_frames, frame_size] (host) -> float32 (int16 with s16) [n_streams, n_frames, 1024, 2]."""
        return self._decode(frames, s16)

    def decode_device(self, frames, out, asynchronous=False, ordered=True):
        """Torch tensors on this decoder's device: frames uint8 [n_streams, n, frame_size] -> out float32 / int16 (s16 output)
        [n_streams, n, 1024, 2]. Ordered behind torch's current stream by default, as At1HipDecoder.decode_device."""
        self._decode_device(frames, out, asynchronous, ordered)


class At3pHipDecoder(_Decoder):
    """n_streams ATRAC3plus streams of 1 or 2 channels decoded side by side on one GPU (include/at3phip.h, the decoder section)."""

    _CODEC, _PREFIX, _COUNTERS = "at3phip", "at3phip_decoder", At3pDecoderCounters

    def __init__(self, n_streams=1, channels=2, max_frames=64, device_id=0, lib_path=None, frame_bytes=None):
        """frame_bytes: the frames' size (at3phip_decoder_set_frame_bytes); None: 2048, and the setter is not called"""
        self.lib = load_library(lib_path)
        self.n_streams, self.channels, self.max_frames = int(n_streams), int(channels), int(max_frames)
        self._create(At3pDecoderConfig(self.channels, self.n_streams, self.max_frames, int(device_id)),
                     "bad configuration, or no usable MI355X / HIP runtime")
        self._frame_bytes = AT3PHIP_FRAME_BYTES
        if frame_bytes is not None:
            self.set_frame_bytes(frame_bytes)

    def set_frame_bytes(self, frame_bytes):
        """at3phip_decoder_set_frame_bytes: waits for queued work; from then on frames are [n_streams, n_frames, frame_bytes]"""
        self._call("set_frame_bytes", int(frame_bytes))
        self._frame_bytes = int(frame_bytes)

    @property
    def frame_bytes(self):
        """at3phip_decoder_get_frame_bytes"""
        v = _I32()
        self._call("get_frame_bytes", ctypes.byref(v))
        return int(v.value)

    def _shapes(self):
        return (self._frame_bytes,), (2048, self.channels)

    def _decode_flags(self, tones, sparse=False):
        """at3phip_decode's flags beside the buffer ones: AT3PHIP_DECODE_TONES for `tones` (a library has tonal-block decoding if it
        has the tone tables) and AT3PHIP_DECODE_SPARSE for `sparse` (include/at3phip.h names at3phip_host_allocate_sparse as the
        symbol that tells a library with SPARSE WORD LENGTHS, encoder and decoder flag alike)."""
        flags = 0
        if sparse:
            _need(self.lib, "at3phip_host_allocate_sparse")
            flags |= AT3PHIP_DECODE_SPARSE
        if tones:
            _need(self.lib, "at3phip_decoder_host_tone_tables")
            flags |= AT3PHIP_DECODE_TONES
        return flags

    def decode(self, frames, s16=False, tones=False, sparse=False):
        """frames uint8 [n_streams, n_frames, frame_bytes] (host) -> float32 (int16 with s16) [n_streams, n_frames, 2048, channels].
        tones: decode tonal blocks (AT3PHIP_DECODE_TONES) instead of rejecting their frames. sparse: decode word length 0 inside the
        coded range (AT3PHIP_DECODE_SPARSE), which AT3PHIP_ALLOC_SPARSE writes, instead of rejecting its frames."""
        return self._decode(frames, s16, self._decode_flags(tones, sparse))

    def decode_device(self, frames, out, asynchronous=False, ordered=True, tones=False, sparse=False):
        """Torch tensors on this decoder's device: frames uint8 [n_streams, n, frame_bytes] -> out float32 / int16 (s16 output)
        [n_streams, n, 2048, channels]. Ordered behind torch's current stream by default, as At1HipDecoder.decode_device.
        tones and sparse as in decode."""
        self._decode_device(frames, out, asynchronous, ordered, self._decode_flags(tones, sparse))


def at3p_decoder_host_tables(lib_path=None):
    """at3phip_decoder_host_tables (no GPU): the decoder's table block as bytes; its first 2048 are the DCT-IV cosines
    double[16][16]."""
    return _host_tables(lib_path, "at3phip_decoder_host_tables", np.zeros(AT3PHIP_DECODER_TABLES_BYTES, np.uint8))


AT3P_TONE_TABLES_DTYPE = np.dtype([("sine", "<f4", 2048), ("hann", "<f4", 256), ("amp_sf", "<f4", 64), ("vlc", "<u2", 16)])
assert AT3P_TONE_TABLES_DTYPE.itemsize == AT3PHIP_DECODER_TONE_TABLES_BYTES


def at3p_decoder_host_tone_tables(lib_path=None):
    """at3phip_decoder_host_tone_tables (no GPU): the tone synthesis' tables as a record of AT3P_TONE_TABLES_DTYPE."""
    return _host_tables(lib_path, "at3phip_decoder_host_tone_tables", np.zeros((), AT3P_TONE_TABLES_DTYPE))


AT3PHIP_RESIDUAL_SCALE = 16
AT3P_TABLES_DTYPE = np.dtype([("fir", "<f4", 384), ("sc32", "<f4", 16), ("sc256", "<f4", 128), ("tw8", "<f4", 16), ("tw64", "<f4", 128),
                              ("sine128", "<f4", 128), ("sine64", "<f4", 64)])
assert AT3P_TABLES_DTYPE.itemsize == 3456


def at3p_host_tables(lib_path=None):
    return _host_tables(lib_path, "at3phip_host_tables", np.zeros((), dtype=AT3P_TABLES_DTYPE))


# at3phip_tonal_block: one frame's tonal block for at3phip_write_frames_tonal (all zero: no tonal block)
AT3P_TONAL_BLOCK_DTYPE = np.dtype([("num_tone_bands", "u1"), ("second_is_leader", "u1"), ("tone_sharing", "<u2"),
                                   ("band", [("n_waves", "u1"), ("start", "u1"), ("stop", "u1"), ("reserved", "u1")], (2, 16)),
                                   ("wave", "<u4", 48)])
assert AT3P_TONAL_BLOCK_DTYPE.itemsize == 324


def pack_tonal_blocks(blocks, channels):
    """Records of AT3P_TONAL_BLOCK_DTYPE, shaped like `blocks`, from (nested lists of) blocks in dict form, None standing for
    "no tonal block": {"nb": NumToneBands, "shared": [nb] bools, "leader": bool, "bands": [ch][nb] {"start": None | 0..31,
    "stop": None | 0..31, "waves": [(FreqIndex, AmpSf, PhaseIndex)]}}. Nothing is checked here (values are masked to their
    fields' widths): the contract is at3phip_write_frames_tonal's."""
    if isinstance(blocks, (list, tuple)):
        return np.stack([pack_tonal_blocks(b, channels) for b in blocks]) if len(blocks) else np.zeros(0, AT3P_TONAL_BLOCK_DTYPE)
    rec = np.zeros((), AT3P_TONAL_BLOCK_DTYPE)
    b = blocks
    if b is None:
        return rec
    nb = int(b["nb"])
    rec["num_tone_bands"] = nb & 0xff
    rec["second_is_leader"] = int(b.get("leader", False)) & 0xff
    rec["tone_sharing"] = sum(int(bool(x)) << i for i, x in enumerate(b.get("shared", [])[:16]))
    at = 0
    for ch in range(channels):
        for i, bd in enumerate(b["bands"][ch][:16]):
            band = rec["band"][ch, i]
            band["n_waves"] = len(bd["waves"]) & 0xff
            band["start"] = 0 if bd["start"] is None else (int(bd["start"]) + 1) & 0xff
            band["stop"] = 0 if bd["stop"] is None else (int(bd["stop"]) + 1) & 0xff
            for fq, sf, ph in bd["waves"]:
                if at < 48:
                    rec["wave"][at] = (int(fq) | int(sf) << 10 | int(ph) << 16) & 0xffffffff
                at += 1
    return rec


# at3phip_host_tone_find_tables: the tone analysis' tables (include/at3phip.h, FINDING TONES); tw is [256][2] (re, im)
AT3P_TONE_FIND_TABLES_DTYPE = np.dtype([("sine", "<f4", 2048), ("hann", "<f4", 256), ("amp_sf", "<f4", 64), ("tw", "<f4", (256, 2)),
                                        ("thr", "<f8", 64), ("rs", "<f8", 1024), ("rc", "<f8", 1024)])
assert AT3P_TONE_FIND_TABLES_DTYPE.itemsize == 28416


def at3p_host_tone_find_tables(lib_path=None):
    """at3phip_host_tone_find_tables (no GPU): the tone analysis' tables as a record of AT3P_TONE_FIND_TABLES_DTYPE."""
    return _host_tables(lib_path, "at3phip_host_tone_find_tables", np.zeros((), AT3P_TONE_FIND_TABLES_DTYPE))


AT3PHIP_TONES_GATED = 32   # flag of the tonal calls: the analysis with envelope points (include/at3phip.h, GATES)


def at3p_host_tone_gates(bands, lib_path=None):
    """at3phip_host_tone_gates (no GPU): bands float32 [F, C, 16, 128] of one stream -> the frames' gates uint8 [F, C, 16]
    (0: none, 1..31: onset at that cell, 0x80 | p: offset with last active cell p). A library without the symbol predates
    AT3PHIP_TONES_GATED."""
    bands = np.ascontiguousarray(bands, dtype=np.float32)
    assert bands.ndim == 4 and bands.shape[1] in (1, 2) and bands.shape[2:] == (16, 128), bands.shape
    out = np.zeros(bands.shape[:3], np.uint8)
    rc = _need(load_library(lib_path), "at3phip_host_tone_gates")(_vp(bands), bands.shape[0], bands.shape[1], _vp(out))
    if rc != 0:
        raise At3HipError(f"at3phip_host_tone_gates failed ({rc})")
    return out


AT3PHIP_ALLOC_ADAPTIVE = 128   # flag of the frame-writing calls: word lengths chosen per frame (include/at3phip.h, ADAPTIVE WORD LENGTHS)
AT3PHIP_TONES_SHARED = 64   # flag of the tonal calls: twin bands of a stereo frame are written once (include/at3phip.h, SHARING)


def at3p_host_tone_flags(lib_path=None):
    """at3phip_host_tone_flags (no GPU): the mask of analysis flags the library understands. A library without the symbol
    predates AT3PHIP_TONES_SHARED."""
    return int(_need(load_library(lib_path), "at3phip_host_tone_flags")())


def _tone_flags(gated, shared):
    return (AT3PHIP_TONES_GATED if gated else 0) | (AT3PHIP_TONES_SHARED if shared else 0)


def _alloc_flag(adaptive, sparse=False, rd=False, psy=False):
    """the allocation flags of a frame-writing call; sparse (AT3PHIP_ALLOC_SPARSE) needs adaptive, rd (AT3PHIP_ALLOC_RD) needs both and psy
    (AT3PHIP_ALLOC_PSY) all three: checked here, before the C call"""
    if psy and not (adaptive and sparse and rd):
        raise ValueError("psy=True needs adaptive=True, sparse=True and rd=True (AT3PHIP_ALLOC_PSY is valid only together with all three)")
    if sparse and not adaptive:
        raise ValueError("sparse=True needs adaptive=True (AT3PHIP_ALLOC_SPARSE is valid only together with AT3PHIP_ALLOC_ADAPTIVE)")
    if rd and not (adaptive and sparse):
        raise ValueError("rd=True needs adaptive=True and sparse=True (AT3PHIP_ALLOC_RD is valid only together with both)")
    return ((AT3PHIP_ALLOC_ADAPTIVE if adaptive else 0) | (AT3PHIP_ALLOC_SPARSE if sparse else 0) | (AT3PHIP_ALLOC_RD if rd else 0)
            | (AT3PHIP_ALLOC_PSY if psy else 0))


def at3p_host_allocate_psy(sfi, bits, dist, tail_bits, frame_bytes=None, offsets=None, lib_path=None):
    """at3phip_host_allocate_psy (no GPU): M1-M6 of include/at3phip.h, MASKING-WEIGHTED WORD LENGTHS, on a cost table and a distortion
    table as at3p_host_allocate_rd takes them; offsets uint8 [C, 32] (each 0..32) are used as given, None: M1-M3 form them
    -> (wl uint8 [C, 32], N, j*, k*, chose_psy, offsets uint8 [C, 32])."""
    sfi, bits, dist = np.ascontiguousarray(sfi, np.uint8), np.ascontiguousarray(bits, np.uint16), np.ascontiguousarray(dist, np.uint64)
    C = sfi.shape[0]
    assert sfi.shape == (C, 32) and bits.shape == (C, 32, 8) and dist.shape == (C, 32, 8), (sfi.shape, bits.shape, dist.shape)
    if offsets is not None:
        offsets = np.ascontiguousarray(offsets, np.uint8)
        assert offsets.shape == (C, 32), offsets.shape
    wl, out, used = np.zeros((C, 32), np.uint8), np.zeros(4, np.int32), np.zeros((C, 32), np.uint8)
    rc = _need(load_library(lib_path), "at3phip_host_allocate_psy")(_vp(sfi), _vp(bits), _vp(dist), None if offsets is None else _vp(offsets), C,
                                                                    int(tail_bits), int(AT3PHIP_FRAME_BYTES if frame_bytes is None else frame_bytes),
                                                                    _vp(wl), _vp(out[0:1]), _vp(out[1:2]), _vp(out[2:3]), _vp(out[3:4]), _vp(used))
    if rc != 0:
        raise At3HipError(f"at3phip_host_allocate_psy failed ({rc})")
    return wl, int(out[0]), int(out[1]), int(out[2]), bool(out[3]), used


def at3p_host_allocate_rd(sfi, bits, dist, tail_bits, frame_bytes=None, lib_path=None):
    """at3phip_host_allocate_rd (no GPU): R2-R4 of include/at3phip.h, RATE-DISTORTION WORD LENGTHS, on a cost table and a distortion
    table: sfi uint8 [C, 32], bits uint16 [C, 32, 8], dist uint64 [C, 32, 8] (S of R1) -> (wl uint8 [C, 32], N, j*, k*, chose_rd)."""
    sfi, bits, dist = np.ascontiguousarray(sfi, np.uint8), np.ascontiguousarray(bits, np.uint16), np.ascontiguousarray(dist, np.uint64)
    C = sfi.shape[0]
    assert sfi.shape == (C, 32) and bits.shape == (C, 32, 8) and dist.shape == (C, 32, 8), (sfi.shape, bits.shape, dist.shape)
    wl, out = np.zeros((C, 32), np.uint8), np.zeros(4, np.int32)
    rc = _need(load_library(lib_path), "at3phip_host_allocate_rd")(_vp(sfi), _vp(bits), _vp(dist), C, int(tail_bits),
                                                                   int(AT3PHIP_FRAME_BYTES if frame_bytes is None else frame_bytes), _vp(wl),
                                                                   _vp(out[0:1]), _vp(out[1:2]), _vp(out[2:3]), _vp(out[3:4]))
    if rc != 0:
        raise At3HipError(f"at3phip_host_allocate_rd failed ({rc})")
    return wl, int(out[0]), int(out[1]), int(out[2]), bool(out[3])


def at3p_host_allocate(sfi, bits, tail_bits, lib_path=None, frame_bytes=None, sparse=False):
    """at3phip_host_allocate (no GPU): steps A3-A5 of include/at3phip.h, ADAPTIVE WORD LENGTHS, on a cost table: sfi uint8 [C, 32],
    bits uint16 [C, 32, 8] (entry w = the unit's bits at word length w) -> (wl uint8 [C, 32], N, t*, k*). frame_bytes: the
    budget's frame size through at3phip_host_allocate_sized; None: the 2048-byte entry point. sparse: A3s and A4s (SPARSE WORD LENGTHS)
    through at3phip_host_allocate_sparse, at frame_bytes or 2048."""
    sfi, bits = np.ascontiguousarray(sfi, np.uint8), np.ascontiguousarray(bits, np.uint16)
    C = sfi.shape[0]
    assert sfi.shape == (C, 32) and bits.shape == (C, 32, 8), (sfi.shape, bits.shape)
    wl, out = np.zeros((C, 32), np.uint8), np.zeros(3, np.int32)
    outs = (_vp(wl), _vp(out[0:1]), _vp(out[1:2]), _vp(out[2:3]))
    if sparse:
        name = "at3phip_host_allocate_sparse"
        rc = _need(load_library(lib_path), name)(_vp(sfi), _vp(bits), C, int(tail_bits), int(AT3PHIP_FRAME_BYTES if frame_bytes is None else frame_bytes), *outs)
    elif frame_bytes is None:
        rc, name = _need(load_library(lib_path), "at3phip_host_allocate")(_vp(sfi), _vp(bits), C, int(tail_bits), *outs), "at3phip_host_allocate"
    else:
        name = "at3phip_host_allocate_sized"
        rc = _need(load_library(lib_path), name)(_vp(sfi), _vp(bits), C, int(tail_bits), int(frame_bytes), *outs)
    if rc != 0:
        raise At3HipError(f"{name} failed ({rc})")
    return wl, int(out[0]), int(out[1]), int(out[2])


class At3pHip(_Context):
    """ATRAC3plus front end (include/at3phip.h): PQF analysis and windowed MDCT-256 x 16 for n_streams streams."""

    _PREFIX = "at3phip"

    def __init__(self, n_streams=1, max_frames=32, channels=2, device_id=0, lib_path=None, frame_bytes=None):
        """frame_bytes: the size of the frames the context writes (at3phip_set_frame_bytes; other than 2048 only with adaptive=True);
        None: 2048, and the setter is not called"""
        self.lib = load_library(lib_path)
        self.channels, self.n_streams = int(channels), int(n_streams)
        self._create(At3pConfig(int(channels), int(n_streams), int(max_frames), int(device_id)), "no usable MI355X / HIP runtime?")
        self._frame_bytes = AT3PHIP_FRAME_BYTES
        if frame_bytes is not None:
            self.set_frame_bytes(frame_bytes)

    def set_frame_bytes(self, frame_bytes):
        """at3phip_set_frame_bytes: waits for queued work; from then on every frame-writing call gives [S, F, frame_bytes]"""
        self._call("set_frame_bytes", int(frame_bytes))
        self._frame_bytes = int(frame_bytes)

    @property
    def frame_bytes(self):
        """at3phip_get_frame_bytes"""
        v = _I32()
        self._call("get_frame_bytes", ctypes.byref(v))
        return int(v.value)

    # one raw method per entry point: pointers (None: absent), a frame count and the function's flags
    def pqf_ptr(self, pcm_ptr, n_frames, bands_ptr, flags):
        self._call("pqf_analyse", ctypes.c_void_p(pcm_ptr), int(n_frames), ctypes.c_void_p(bands_ptr), int(flags))

    def mdct_ptr(self, bands_ptr, n_frames, win_flags_ptr, specs_ptr, flags):
        self._call("mdct", ctypes.c_void_p(bands_ptr), int(n_frames), ctypes.c_void_p(win_flags_ptr), ctypes.c_void_p(specs_ptr),
                   int(flags))

    def pqf_mdct_ptr(self, pcm_ptr, n_frames, win_flags_ptr, bands_ptr, specs_ptr, flags):
        self._call("pqf_mdct", ctypes.c_void_p(pcm_ptr), int(n_frames), ctypes.c_void_p(win_flags_ptr), ctypes.c_void_p(bands_ptr),
                   ctypes.c_void_p(specs_ptr), int(flags))

    def write_frames_ptr(self, specs_ptr, n_frames, win_flags_ptr, frames_ptr, flags):
        self._call("write_frames", ctypes.c_void_p(specs_ptr), int(n_frames), ctypes.c_void_p(win_flags_ptr),
                   ctypes.c_void_p(frames_ptr), int(flags))

    def write_frames_tonal_ptr(self, specs_ptr, n_frames, win_flags_ptr, tonal_ptr, frames_ptr, flags):
        self._call("write_frames_tonal", ctypes.c_void_p(specs_ptr), int(n_frames), ctypes.c_void_p(win_flags_ptr),
                   ctypes.c_void_p(tonal_ptr), ctypes.c_void_p(frames_ptr), int(flags))

    def encode_frames_ptr(self, pcm_ptr, n_frames, frames_ptr, flags):
        """Raw pointers (float32 PCM) and at3phip_encode_frames flags."""
        self._call("encode_frames", ctypes.c_void_p(pcm_ptr), int(n_frames), ctypes.c_void_p(frames_ptr), int(flags))

    def encode_frames_s16_ptr(self, pcm_ptr, n_frames, frames_ptr, flags):
        """Raw pointers (int16 PCM, 2-byte alignment is enough) and at3phip_encode_frames_short flags."""
        self._call("encode_frames_short", ctypes.c_void_p(pcm_ptr), int(n_frames), ctypes.c_void_p(frames_ptr), int(flags))

    def analyse_tones_ptr(self, bands_ptr, n_frames, blocks_ptr, residual_ptr, flags):
        """Raw pointers (the records are host memory; None: not wanted) and at3phip_analyse_tones flags."""
        self._call("analyse_tones", ctypes.c_void_p(bands_ptr), int(n_frames), ctypes.c_void_p(blocks_ptr), ctypes.c_void_p(residual_ptr),
                   int(flags))

    def encode_frames_tonal_ptr(self, pcm_ptr, n_frames, frames_ptr, flags):
        """Raw pointers (float32 PCM) and at3phip_encode_frames_tonal flags."""
        self._call("encode_frames_tonal", ctypes.c_void_p(pcm_ptr), int(n_frames), ctypes.c_void_p(frames_ptr), int(flags))

    def encode_frames_tonal_s16_ptr(self, pcm_ptr, n_frames, frames_ptr, flags):
        """Raw pointers (int16 PCM) and at3phip_encode_frames_tonal_short flags."""
        self._call("encode_frames_tonal_short", ctypes.c_void_p(pcm_ptr), int(n_frames), ctypes.c_void_p(frames_ptr), int(flags))

    def _flags(self, win_flags, nf):
        """win_flags as uint16 [n_streams, nf, channels] (kept alive by the caller) and its address, or (None, None)"""
        if win_flags is None:
            return None, None
        fl = np.ascontiguousarray(win_flags, dtype=np.uint16)
        assert fl.shape == (self.n_streams, nf, self.channels), fl.shape
        return fl, fl.ctypes.data

    def pqf(self, pcm):
        """pcm float32 [S, F, 2048, C] -> subbands [S, F, C, 16, 128]."""
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        assert pcm.ndim == 4 and pcm.shape[0] == self.n_streams and pcm.shape[2:] == (2048, self.channels), pcm.shape
        out = np.zeros((self.n_streams, pcm.shape[1], self.channels, 16, 128), np.float32)
        self.pqf_ptr(pcm.ctypes.data, pcm.shape[1], out.ctypes.data, 0)
        return out

    def mdct(self, bands, win_flags=None, residual_scale=False):
        """bands [S, F, C, 16, 128], win_flags uint16 [S, F, C] or None -> specs [S, F, C, 2048]."""
        bands = np.ascontiguousarray(bands, dtype=np.float32)
        nf = bands.shape[1]
        fl, flp = self._flags(win_flags, nf)
        out = np.zeros((self.n_streams, nf, self.channels, 2048), np.float32)
        self.mdct_ptr(bands.ctypes.data, nf, flp, out.ctypes.data, AT3PHIP_RESIDUAL_SCALE if residual_scale else 0)
        return out

    def pqf_mdct(self, pcm, win_flags=None, residual_scale=False, want_bands=True):
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        nf = pcm.shape[1]
        fl, flp = self._flags(win_flags, nf)
        bands = np.zeros((self.n_streams, nf, self.channels, 16, 128), np.float32) if want_bands else None
        specs = np.zeros((self.n_streams, nf, self.channels, 2048), np.float32)
        self.pqf_mdct_ptr(pcm.ctypes.data, nf, flp, bands.ctypes.data if want_bands else None, specs.ctypes.data,
                          AT3PHIP_RESIDUAL_SCALE if residual_scale else 0)
        return bands, specs

    def pqf_mdct_device(self, pcm_ptr, n_frames, specs_ptr):
        self.pqf_mdct_ptr(pcm_ptr, n_frames, None, None, specs_ptr, _device_flags(False))

    def write_frames(self, specs, win_flags=None, tonal=None, adaptive=False, sparse=False, rd=False, psy=False):
        """ScaleFrame + WriteFrame: specs [S, F, C, 2048], win_flags uint16 [S, F, C] or None, tonal records of
        AT3P_TONAL_BLOCK_DTYPE [S, F] (pack_tonal_blocks) or None: no frame carries a tonal block (at3phip_write_frames)
        -> frames uint8 [S, F, frame_bytes]. adaptive: AT3PHIP_ALLOC_ADAPTIVE, word lengths chosen per frame to fill it."""
        specs = np.ascontiguousarray(specs, dtype=np.float32)
        assert specs.ndim == 4 and specs.shape[0] == self.n_streams and specs.shape[2:] == (self.channels, 2048), specs.shape
        nf = specs.shape[1]
        fl, flp = self._flags(win_flags, nf)
        out = np.zeros((self.n_streams, nf, self._frame_bytes), np.uint8)
        if tonal is None:
            self.write_frames_ptr(specs.ctypes.data, nf, flp, out.ctypes.data, _alloc_flag(adaptive, sparse, rd, psy))
        else:
            tonal = np.ascontiguousarray(tonal, dtype=AT3P_TONAL_BLOCK_DTYPE)
            assert tonal.shape == (self.n_streams, nf), tonal.shape
            self.write_frames_tonal_ptr(specs.ctypes.data, nf, flp, tonal.ctypes.data, out.ctypes.data, _alloc_flag(adaptive, sparse, rd, psy))
        return out

    def _encode_frames_host(self, pcm, dtype, raw, flags=0):
        pcm = np.ascontiguousarray(pcm, dtype=dtype)
        assert pcm.ndim == 4 and pcm.shape[0] == self.n_streams and pcm.shape[2:] == (2048, self.channels), pcm.shape
        nf = pcm.shape[1]
        out = np.zeros((self.n_streams, nf, self._frame_bytes), np.uint8)
        raw(pcm.ctypes.data, nf, out.ctypes.data, flags)
        return out

    def encode_frames(self, pcm, adaptive=False, sparse=False, rd=False, psy=False):
        """pcm float32 [S, F, 2048, C] -> frames uint8 [S, F, frame_bytes] (tonal analysis finding nothing; no look-ahead delay).
        adaptive (here and in the encode calls below): AT3PHIP_ALLOC_ADAPTIVE, word lengths chosen per frame to fill it."""
        return self._encode_frames_host(pcm, np.float32, self.encode_frames_ptr, _alloc_flag(adaptive, sparse, rd, psy))

    def encode_frames_s16(self, pcm, adaptive=False, sparse=False, rd=False, psy=False):
        """pcm int16 [S, F, 2048, C] (host) -> frames uint8 [S, F, 2048] (at3phip_encode_frames_short): the frames of
        encode_frames() on pcm / 32768 as float32, bit for bit; the samples cross the bus as 16-bit and are widened by the
        filter bank. Calls of both kinds may alternate."""
        return self._encode_frames_host(pcm, np.int16, self.encode_frames_s16_ptr, _alloc_flag(adaptive, sparse, rd, psy))

    def analyse_tones(self, bands, gated=False, shared=False):
        """bands float32 [S, F, C, 16, 128] (what pqf() returns) -> (blocks of AT3P_TONAL_BLOCK_DTYPE [S, F], residual
        [S, F, C, 16, 128]): at3phip_analyse_tones, slot f holding the block of (frame f-1, frame f) and the residual of frame
        f-1; the last frame and block carry over to the next call. gated: AT3PHIP_TONES_GATED, onsets and offsets become the
        records' envelope points; shared: AT3PHIP_TONES_SHARED, a band that both channels of a stereo frame hold identically is
        written and counted once (a stream stays with one mode between resets)."""
        bands = np.ascontiguousarray(bands, dtype=np.float32)
        assert bands.ndim == 5 and bands.shape[0] == self.n_streams and bands.shape[2:] == (self.channels, 16, 128), bands.shape
        nf = bands.shape[1]
        blocks = np.zeros((self.n_streams, nf), AT3P_TONAL_BLOCK_DTYPE)
        resid = np.zeros_like(bands)
        self.analyse_tones_ptr(bands.ctypes.data, nf, blocks.ctypes.data, resid.ctypes.data, _tone_flags(gated, shared))
        return blocks, resid

    def analyse_tones_device(self, bands_ptr, n_frames, residual_ptr, gated=False, shared=False):
        """Device-resident subband samples and residual (raw pointers) -> the blocks [S, F] (host memory). The call waits; whatever
        produces the samples must be complete before it (see encode_frames_device)."""
        blocks = np.zeros((self.n_streams, int(n_frames)), AT3P_TONAL_BLOCK_DTYPE)
        self.analyse_tones_ptr(bands_ptr, n_frames, blocks.ctypes.data, residual_ptr, _device_flags(False) | _tone_flags(gated, shared))
        return blocks

    def encode_frames_tonal(self, pcm, gated=False, shared=False, adaptive=False, sparse=False, rd=False, psy=False):
        """pcm float32 [S, F, 2048, C] -> frames uint8 [S, F, 2048] with the tone analysis (at3phip_encode_frames_tonal): frame f
        of the stream holds the residual of input frame f-1 and the block of frame f-2, so one trailing frame of silence flushes.
        gated: AT3PHIP_TONES_GATED, shared: AT3PHIP_TONES_SHARED, as in analyse_tones()."""
        return self._encode_frames_host(pcm, np.float32, self.encode_frames_tonal_ptr, _tone_flags(gated, shared) | _alloc_flag(adaptive, sparse, rd, psy))

    def encode_frames_tonal_s16(self, pcm, gated=False, shared=False, adaptive=False, sparse=False, rd=False, psy=False):
        """The same for int16 PCM (at3phip_encode_frames_tonal_short): the frames of encode_frames_tonal() on pcm / 32768."""
        return self._encode_frames_host(pcm, np.int16, self.encode_frames_tonal_s16_ptr, _tone_flags(gated, shared) | _alloc_flag(adaptive, sparse, rd, psy))

    def encode_frames_tonal_device(self, pcm_ptr, n_frames, frames_ptr, asynchronous=False, gated=False, shared=False, adaptive=False, sparse=False, rd=False, psy=False):
        """Device-resident float32 PCM / frames; ordering and what stays untouched until sync() as in encode_frames_device."""
        self.encode_frames_tonal_ptr(pcm_ptr, n_frames, frames_ptr, _device_flags(asynchronous) | _tone_flags(gated, shared) | _alloc_flag(adaptive, sparse, rd, psy))

    def encode_frames_tonal_device_s16(self, pcm_ptr, n_frames, frames_ptr, asynchronous=False, gated=False, shared=False, adaptive=False, sparse=False, rd=False, psy=False):
        """Device-resident int16 PCM / frames, as encode_frames_tonal_device."""
        self.encode_frames_tonal_s16_ptr(pcm_ptr, n_frames, frames_ptr, _device_flags(asynchronous) | _tone_flags(gated, shared) | _alloc_flag(adaptive, sparse, rd, psy))

    def encode_frames_device(self, pcm_ptr, n_frames, frames_ptr, asynchronous=False, adaptive=False, sparse=False, rd=False, psy=False):
        """asynchronous=True only queues the call (AT3HIP_ASYNC): sync() before the frames are read, and both buffers stay
        untouched until then. The context's streams are non-blocking (at3hip.h, DEVICE BUFFERS AND STREAMS): they wait for no
        other stream, so whatever produces the PCM must be complete before the call."""
        self.encode_frames_ptr(pcm_ptr, n_frames, frames_ptr, _device_flags(asynchronous) | _alloc_flag(adaptive, sparse, rd, psy))

    def encode_frames_device_s16(self, pcm_ptr, n_frames, frames_ptr, asynchronous=False, adaptive=False, sparse=False, rd=False, psy=False):
        """Device-resident int16 PCM / frames (raw pointers; the PCM needs only 2-byte alignment). Stream ordering and what
        stays untouched until sync() as in encode_frames_device."""
        self.encode_frames_s16_ptr(pcm_ptr, n_frames, frames_ptr, _device_flags(asynchronous) | _alloc_flag(adaptive, sparse, rd, psy))

    def timings(self):
        a, b, w = ctypes.c_float(), ctypes.c_float(), ctypes.c_float()
        self._call("get_timings", ctypes.byref(a), ctypes.byref(b))
        self._call("get_write_timing", ctypes.byref(w))
        return {"pqf_ms": a.value, "mdct_ms": b.value, "write_ms": w.value}


def resampler_shape(in_rate, out_rate, lib_path=None):
    """at3hip_resampler_shape (no GPU): (L phases, M input step, K taps per phase) of a supported pair."""
    L, M, K = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    _lib_call(lib_path, "at3hip_resampler_shape", int(in_rate), int(out_rate), ctypes.byref(L), ctypes.byref(M), ctypes.byref(K),
              why=f": {in_rate} -> {out_rate} is an unsupported pair")
    return L.value, M.value, K.value


def resampler_host_tables(in_rate, out_rate, lib_path=None):
    """at3hip_resampler_host_tables (no GPU): the filter table hp float32 [L][K] as at3hip_resampler_create builds it."""
    L, _, K = resampler_shape(in_rate, out_rate, lib_path)
    return _host_tables(lib_path, "at3hip_resampler_host_tables", np.zeros((L, K), np.float32), int(in_rate), int(out_rate))


class HipResampler(_Context):
    """n_streams streams of 1 or 2 channels converted from in_rate to out_rate side by side on one GPU
    (include/at3hip_resample.h). Every stream of a call takes the same number of input samples."""

    _PREFIX = "at3hip_resampler"

    def __init__(self, in_rate, out_rate, channels=2, n_streams=1, max_in=1 << 16, device_id=0, lib_path=None):
        self.lib = load_library(lib_path)
        self.in_rate, self.out_rate = int(in_rate), int(out_rate)
        self.channels, self.n_streams, self.max_in = int(channels), int(n_streams), int(max_in)
        self._create(ResamplerConfig(self.in_rate, self.out_rate, self.channels, self.n_streams, self.max_in, int(device_id)),
                     "unsupported rates or configuration, or no usable MI355X / HIP runtime")
        self.max_out = int(self._value("max_out"))
        self.L, self.M, self.K = resampler_shape(self.in_rate, self.out_rate, lib_path)

    def process_ptr(self, in_ptr, n_in, out_ptr, flags):
        """Raw pointers and at3hip_resampler_process flags (AT3HIP_RESAMPLE_OUT_S16: out is int16); returns the outputs per
        stream. The resampler's stream is non-blocking (at3hip.h, DEVICE BUFFERS AND STREAMS): it waits for no other stream, so
        whatever produces a device buffer must be complete before the call (or share the stream given to set_stream)."""
        n = ctypes.c_int32()
        self._call("process", ctypes.c_void_p(in_ptr), int(n_in), ctypes.c_void_p(out_ptr), ctypes.byref(n), int(flags))
        return n.value

    def process_s16_ptr(self, in_ptr, n_in, out_ptr, flags):
        """Raw pointers and at3hip_resampler_process_s16 flags (int16 input, 2-byte alignment is enough; out float32, or int16
        with AT3HIP_RESAMPLE_OUT_S16); returns the outputs per stream. Stream ordering as in process_ptr, and with AT3HIP_ASYNC
        the buffers stay untouched until sync()."""
        n = ctypes.c_int32()
        self._call("process_s16", ctypes.c_void_p(in_ptr), int(n_in), ctypes.c_void_p(out_ptr), ctypes.byref(n), int(flags))
        return n.value

    def flush_ptr(self, out_ptr, flags):
        n = ctypes.c_int32()
        self._call("flush", ctypes.c_void_p(out_ptr), ctypes.byref(n), int(flags))
        return n.value

    def _host_out(self, out_s16):
        return np.zeros((self.n_streams, self.max_out, self.channels), np.int16 if out_s16 else np.float32)

    def _trim(self, out, n):
        return np.ascontiguousarray(out.reshape(-1)[: self.n_streams * n * self.channels].reshape(self.n_streams, n, self.channels))

    def _process_host(self, pcm, dtype, raw, out_s16):
        pcm = np.ascontiguousarray(pcm, dtype=dtype)
        assert pcm.ndim == 3 and pcm.shape[0] == self.n_streams and pcm.shape[2] == self.channels, pcm.shape
        out = self._host_out(out_s16)
        n = raw(pcm.ctypes.data, pcm.shape[1], out.ctypes.data, AT3HIP_RESAMPLE_OUT_S16 if out_s16 else 0)
        return self._trim(out, n)

    def process(self, pcm, out_s16=False):
        """pcm float32 [n_streams, n_in, channels] (host) -> float32 [n_streams, n_out, channels]; with out_s16=True int16,
        lrintf(clamp(x, -1, 1) * 32767) of the float output (AT3HIP_RESAMPLE_OUT_S16). A blocking call on the resampler's own
        non-blocking stream (at3hip.h, DEVICE BUFFERS AND STREAMS): host memory in, host memory out, complete on return."""
        return self._process_host(pcm, np.float32, self.process_ptr, out_s16)

    def process_s16(self, pcm, out_s16=False):
        """pcm int16 [n_streams, n_in, channels] (host) -> what process() gives on pcm / 32768 as float32, bit for bit
        (at3hip_resampler_process_s16): the samples cross the bus as 16-bit and are widened by the kernel. Calls of both kinds
        may alternate. Blocking, as process()."""
        return self._process_host(pcm, np.int16, self.process_s16_ptr, out_s16)

    def flush(self, out_s16=False):
        """The remaining outputs of every stream, float32 (int16 with out_s16=True) [n_streams, n_out, channels]; then the start
        state. Blocking, as process()."""
        out = self._host_out(out_s16)
        n = self.flush_ptr(out.ctypes.data, AT3HIP_RESAMPLE_OUT_S16 if out_s16 else 0)
        return self._trim(out, n)

    def _device_out(self, out, device):
        import torch
        assert out.dtype == torch.float32 and out.is_contiguous() and out.device == device
        assert out.numel() >= self.n_streams * self.max_out * self.channels, tuple(out.shape)

    def process_device(self, pcm, out, asynchronous=False, ordered=True):
        """Torch tensors on this resampler's device: pcm float32 [n_streams, n_in, channels] -> out float32 with room for
        max_out samples per stream; outputs are written as [n_streams][n][channels] from out's start. Returns n. Ordered
        behind torch's current stream by default, as the decoders' decode_device."""
        import torch
        assert pcm.dtype == torch.float32 and pcm.is_contiguous()
        assert pcm.ndim == 3 and pcm.shape[0] == self.n_streams and pcm.shape[2] == self.channels, tuple(pcm.shape)
        self._device_out(out, pcm.device)
        self._order_behind_torch(pcm.device, ordered)
        return self.process_ptr(pcm.data_ptr(), pcm.shape[1], out.data_ptr(), _device_flags(asynchronous))

    def flush_device(self, out, asynchronous=False, ordered=True):
        """flush into a torch tensor, as process_device; returns n."""
        self._device_out(out, out.device)
        self._order_behind_torch(out.device, ordered)
        return self.flush_ptr(out.data_ptr(), AT3HIP_OUT_ON_DEVICE | (AT3HIP_ASYNC if asynchronous else 0))


def loudness_gate(z, lib_path=None):
    """at3hip_loudness_gate (no GPU): hop sums z float64 [n_hops][channels] -> LoudnessResult with integrated, momentary_max,
    short_term_max, n_hops and n_blocks_kept set (peaks and n_samples zero)."""
    z = np.ascontiguousarray(z, np.float64)
    assert z.ndim == 2 and z.shape[1] in (1, 2), z.shape
    r = LoudnessResult()
    _lib_call(lib_path, "at3hip_loudness_gate", _vp(z), z.shape[0], z.shape[1], ctypes.byref(r))
    return r


def loudness_gain(result, target_lufs, ceiling_db=-1.0, lib_path=None):
    """at3hip_loudness_gain (no GPU): the float32 gain that brings `result` (a LoudnessResult) to target_lufs with its peak
    (the true peak if it was measured, else the sample peak) at or below ceiling_db dBFS; 1.0 for a stream without loudness."""
    g = ctypes.c_float()
    if not isinstance(result, LoudnessResult):   # (a structure of the same layout)
        result = LoudnessResult.from_buffer_copy(bytes(result))
    _lib_call(lib_path, "at3hip_loudness_gain", ctypes.byref(result), float(target_lufs), float(ceiling_db), ctypes.byref(g))
    return np.float32(g.value)


class HipLoudness(_Context):
    """n_streams streams of 1 or 2 channels at 44.1 kHz metered side by side on one GPU (include/at3hip_loudness.h): BS.1770
    hop sums, sample peak and, with true_peak=True, the 4x oversampled peak; finish() gates on the host. Every stream of a call
    takes the same number of samples.

    Stream ordering (at3hip.h, DEVICE BUFFERS AND STREAMS): the meter reads and writes device buffers on its own non-blocking
    stream, which waits for no other stream. The *_device methods therefore queue the call on torch's current stream by
    default (ordered=True, through at3hip_loudness_set_stream; on the null stream they wait for it instead); with ordered=False
    whatever produces the buffer must be complete before the call. With asynchronous=True the buffers must stay valid until
    sync() or finish()."""

    _PREFIX = "at3hip_loudness"

    def __init__(self, channels=2, n_streams=1, max_in=1 << 16, max_hops=36000, true_peak=False, device_id=0, lib_path=None):
        self.lib = load_library(lib_path)
        self.channels, self.n_streams, self.max_in, self.max_hops = int(channels), int(n_streams), int(max_in), int(max_hops)
        self.true_peak = bool(true_peak)
        self.n_samples = 0   # per stream since the start / the last finish() or reset()
        self._create(LoudnessConfig(self.channels, self.n_streams, self.max_in, self.max_hops, int(self.true_peak), int(device_id)),
                     "unsupported configuration, or no usable MI355X / HIP runtime")

    def reset(self):
        self._call("reset")
        self.n_samples = 0

    def process_ptr(self, in_ptr, n_in, flags):
        """Raw pointer and at3hip_loudness_process flags."""
        self._call("process", ctypes.c_void_p(in_ptr), int(n_in), int(flags))
        self.n_samples += int(n_in)

    def process_s16_ptr(self, in_ptr, n_in, flags):
        """Raw pointer (int16 samples, 2-byte alignment is enough) and at3hip_loudness_process_s16 flags; stream ordering as in
        the class docstring: the meter's non-blocking stream waits for no other stream."""
        self._call("process_s16", ctypes.c_void_p(in_ptr), int(n_in), int(flags))
        self.n_samples += int(n_in)

    def _host_pcm(self, pcm, dtype):
        pcm = np.ascontiguousarray(pcm, dtype=dtype)
        assert pcm.ndim == 3 and pcm.shape[0] == self.n_streams and pcm.shape[2] == self.channels, pcm.shape
        return pcm

    def process(self, pcm):
        """pcm float32 [n_streams, n_in, channels] (host)"""
        pcm = self._host_pcm(pcm, np.float32)
        self.process_ptr(pcm.ctypes.data, pcm.shape[1], 0)

    def process_s16(self, pcm):
        """pcm int16 [n_streams, n_in, channels] (host): what process() measures on pcm / 32768 as float32, bit for bit
        (at3hip_loudness_process_s16); the samples cross the bus as 16-bit and are widened by the kernels. Calls of both kinds
        may alternate. A blocking call on the meter's own non-blocking stream (see the class docstring). Measured: the meter is
        compute-bound and its hop kernel takes 1.5 times as long on 16-bit samples, so from host memory this is 1.1 times as
        fast as process(), and on device-resident floats process_device() is the faster call."""
        pcm = self._host_pcm(pcm, np.int16)
        self.process_s16_ptr(pcm.ctypes.data, pcm.shape[1], 0)

    def process_device(self, pcm, asynchronous=False, ordered=True):
        """pcm: torch float32 [n_streams, n_in, channels] on this meter's device (see the class docstring for the ordering)."""
        import torch
        assert pcm.dtype == torch.float32 and pcm.is_contiguous()
        assert pcm.ndim == 3 and pcm.shape[0] == self.n_streams and pcm.shape[2] == self.channels, tuple(pcm.shape)
        self._order_behind_torch(pcm.device, ordered)
        self.process_ptr(pcm.data_ptr(), pcm.shape[1], AT3HIP_PCM_ON_DEVICE | (AT3HIP_ASYNC if asynchronous else 0))

    def hops(self):
        """the hop sums so far, float64 [n_streams, n_hops, channels] (at3hip_loudness_read_hops; waits for queued work)"""
        out = np.zeros((self.n_streams, self.n_samples // LOUDNESS_HOP, self.channels), np.float64)
        for s in range(self.n_streams):
            self._call("read_hops", s, _vp(out[s]), out[s].nbytes)
        return out

    def finish(self):
        """Waits, gates, and returns one LoudnessResult per stream; the meter is then at its start state."""
        res = (LoudnessResult * self.n_streams)()
        self._call("finish", res)
        self.n_samples = 0
        return list(res)

    def _gains(self, gains):
        gains = np.ascontiguousarray(gains, np.float32)
        assert gains.shape == (self.n_streams,), gains.shape
        return gains

    def apply_ptr(self, in_ptr, n_in, gains, out_ptr, flags):
        gains = self._gains(gains)
        self._call("apply", ctypes.c_void_p(in_ptr), int(n_in), _vp(gains), ctypes.c_void_p(out_ptr), int(flags))

    def apply_s16_ptr(self, in_ptr, n_in, gains, out_ptr, flags):
        """Raw pointers (int16 in, float32 out) and at3hip_loudness_apply_s16 flags; stream ordering as in the class docstring."""
        gains = self._gains(gains)
        self._call("apply_s16", ctypes.c_void_p(in_ptr), int(n_in), _vp(gains), ctypes.c_void_p(out_ptr), int(flags))

    def _apply_host(self, pcm, gains, dtype, raw):
        pcm = self._host_pcm(pcm, dtype)
        out = np.zeros(pcm.shape, np.float32)
        raw(pcm.ctypes.data, pcm.shape[1], gains, out.ctypes.data, 0)
        return out

    def apply(self, pcm, gains):
        """pcm float32 [n_streams, n_in, channels] (host), gains float32 [n_streams] -> pcm * gains[:, None, None] as float32"""
        return self._apply_host(pcm, gains, np.float32, self.apply_ptr)

    def apply_s16(self, pcm, gains):
        """pcm int16 [n_streams, n_in, channels] (host), gains float32 [n_streams] -> (pcm / 32768 as float32) * gains[:, None, None]
        as float32 (at3hip_loudness_apply_s16). A blocking call on the meter's own non-blocking stream (see the class docstring)."""
        return self._apply_host(pcm, gains, np.int16, self.apply_s16_ptr)

    def apply_device(self, pcm, gains, out, asynchronous=False, ordered=True):
        """Torch tensors on this meter's device: out = pcm * gains[stream] (out may be pcm); ordering as process_device."""
        import torch
        assert pcm.dtype == torch.float32 and pcm.is_contiguous() and out.dtype == torch.float32 and out.is_contiguous()
        assert pcm.ndim == 3 and pcm.shape[0] == self.n_streams and pcm.shape[2] == self.channels, tuple(pcm.shape)
        assert out.device == pcm.device and out.numel() >= pcm.numel()
        self._order_behind_torch(pcm.device, ordered)
        self.apply_ptr(pcm.data_ptr(), pcm.shape[1], gains, out.data_ptr(), _device_flags(asynchronous))

    # ---- the look-ahead limiter (at3hip_loudness.h, "The look-ahead limiter") ----
    def limit_delay(self, true_peak=False):
        """the latency in samples (at3hip_loudness_limit_delay; no GPU)"""
        return int(_need(self.lib, "at3hip_loudness_limit_delay")(AT3HIP_LIMIT_TRUE_PEAK if true_peak else 0))

    def limit_start(self, gains, ceiling, true_peak=False):
        """Begins a limiter run: gains float32 [n_streams] (finite, >= 0), ceiling linear (finite, > 0), detector on the samples
        or, with true_peak, on the 4x oversampled signal too. The run lasts until limit_flush() or reset()."""
        gains = self._gains(gains)
        self._call("limit_start", _vp(gains), ctypes.c_float(ceiling), AT3HIP_LIMIT_TRUE_PEAK if true_peak else 0)

    def limit_ptr(self, in_ptr, n_in, out_ptr, flags, s16=False):
        """Raw pointers and at3hip_loudness_limit (or, with s16, _limit_s16) flags; returns the outputs per stream."""
        n = ctypes.c_int32()
        self._call("limit_s16" if s16 else "limit", ctypes.c_void_p(in_ptr), int(n_in), ctypes.c_void_p(out_ptr), ctypes.byref(n), int(flags))
        return n.value

    def limit_flush_ptr(self, out_ptr, flags):
        n = ctypes.c_int32()
        self._call("limit_flush", ctypes.c_void_p(out_ptr), ctypes.byref(n), int(flags))
        return n.value

    def _limit_host(self, pcm, dtype):
        pcm = self._host_pcm(pcm, dtype)
        out = np.zeros(pcm.shape, np.float32)
        n = self.limit_ptr(pcm.ctypes.data, pcm.shape[1], out.ctypes.data, 0, s16=dtype is np.int16)
        return np.ascontiguousarray(out.reshape(-1)[: self.n_streams * n * self.channels].reshape(self.n_streams, n, self.channels))

    def limit(self, pcm):
        """pcm float32 [n_streams, n_in, channels] (host) -> the outputs this call completes, float32 [n_streams, n_out, channels]
        (n_out <= n_in: the limiter holds back limit_delay() samples until limit_flush)"""
        return self._limit_host(pcm, np.float32)

    def limit_s16(self, pcm):
        """limit() for int16 samples, taken as pcm / 32768 in float32 (at3hip_loudness_limit_s16); the output is float32"""
        return self._limit_host(pcm, np.int16)

    def limit_flush(self):
        """the held-back outputs, float32 [n_streams, n_out, channels]; ends the run (limit_stats() stays readable)"""
        out = np.zeros((self.n_streams, LIMIT_LOOKAHEAD + 72, self.channels), np.float32)
        n = self.limit_flush_ptr(out.ctypes.data, 0)
        return np.ascontiguousarray(out.reshape(-1)[: self.n_streams * n * self.channels].reshape(self.n_streams, n, self.channels))

    def limit_stats(self):
        """one LimitStats per stream for the run begun by the last limit_start (waits for queued work)"""
        st = (LimitStats * self.n_streams)()
        self._call("limit_stats", st)
        return list(st)

    def limit_device(self, pcm, out, asynchronous=False, ordered=True):
        """Torch tensors on this meter's device: pcm float32 or int16 [n_streams, n_in, channels]; out float32, contiguous, with
        room for n_streams * n_in * channels values, not overlapping pcm. Returns n_out: the outputs are out's first
        n_streams * n_out * channels values as [n_streams, n_out, channels]. Ordering as process_device."""
        import torch
        assert pcm.dtype in (torch.float32, torch.int16) and pcm.is_contiguous() and out.dtype == torch.float32 and out.is_contiguous()
        assert pcm.ndim == 3 and pcm.shape[0] == self.n_streams and pcm.shape[2] == self.channels, tuple(pcm.shape)
        assert out.device == pcm.device and out.numel() >= pcm.numel()
        self._order_behind_torch(pcm.device, ordered)
        return self.limit_ptr(pcm.data_ptr(), pcm.shape[1], out.data_ptr(), _device_flags(asynchronous), s16=pcm.dtype == torch.int16)

    def limit_flush_device(self, out, asynchronous=False, ordered=True):
        """limit_flush into a torch float32 tensor with room for n_streams * limit_delay() * channels values; returns n_out."""
        import torch
        assert out.dtype == torch.float32 and out.is_contiguous()
        self._order_behind_torch(out.device, ordered)
        return self.limit_flush_ptr(out.data_ptr(), AT3HIP_OUT_ON_DEVICE | (AT3HIP_ASYNC if asynchronous else 0))
