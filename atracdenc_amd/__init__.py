"""atracdenc_amd: MI355X-native ATRAC3 / ATRAC1 / ATRAC3plus encode hot paths and ATRAC1 / ATRAC3 decoders, a batched sample-rate converter and a batched loudness meter.

Python is only the test/bench harness around the C-ABI library (include/at3hip.h); the product is
libat3hip.so (hand-written HIP for gfx950, atracdenc_amd/csrc). There is no CPU fallback: importing
works anywhere, but creating an encoder raises if the library or a GPU is missing.
"""
from .binding import At1Hip, At1HipDecoder, At3Hip, At3HipDecoder, At3pHip, At3pHipDecoder, At3HipError, HipLoudness, HipResampler, LIB_PATH, build_library, load_library, loudness_gain, loudness_gate, resampler_host_tables  # noqa: F401

__all__ = ["At1Hip", "At1HipDecoder", "At3Hip", "At3HipDecoder", "At3pHip", "At3pHipDecoder", "At3HipError", "HipLoudness", "HipResampler", "LIB_PATH", "build_library", "load_library", "loudness_gain", "loudness_gate", "resampler_host_tables"]
