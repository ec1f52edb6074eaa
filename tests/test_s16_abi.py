"""The 16-bit PCM entry points are part of the exported C ABI (no compute without a GPU): the five functions are exported and
listed where tests/test_abi.py looks for them, the output flag has the decoders' bit, and the reported ABI version stays 1.6."""
import os
import re

import atracdenc_amd
from atracdenc_amd import binding

AT3HIP = ("at3hip_resampler_process_s16", "at3hip_loudness_process_s16", "at3hip_loudness_apply_s16")
INCLUDE = os.path.join(os.path.dirname(atracdenc_amd.__file__), "..", "include")


def _lib():
    if not os.path.exists(atracdenc_amd.LIB_PATH):
        atracdenc_amd.build_library()
    return atracdenc_amd.load_library()


def test_s16_entry_points_are_exported():
    lib = _lib()
    for name in AT3HIP + ("at1hip_encode_short", "at3phip_encode_frames_short"):
        assert hasattr(lib, name), name


def test_s16_entry_points_are_listed():
    for name in AT3HIP:
        assert name in binding.SYMBOLS, name
    assert "at1hip_encode_short" in binding.AT1_SYMBOLS
    assert "at3phip_encode_frames_short" in binding.AT3P_SYMBOLS


def test_s16_entry_points_are_declared():
    """each in its engine's header, and the at3hip_* ones in at3hip.h's version notes"""
    for header, names in (("at1hip.h", ("at1hip_encode_short",)), ("at3phip.h", ("at3phip_encode_frames_short",)),
                          ("at3hip_resample.h", AT3HIP[:1]), ("at3hip_loudness.h", AT3HIP[1:]), ("at3hip.h", AT3HIP)):
        text = open(os.path.join(INCLUDE, header)).read()
        for name in names:
            assert re.search(r"\b" + name + r"\s*\(", text), (header, name)


def test_resample_out_s16_is_the_decoders_bit():
    text = open(os.path.join(INCLUDE, "at3hip_resample.h")).read()
    assert re.search(r"#define\s+AT3HIP_RESAMPLE_OUT_S16\s+8u\b", text)
    assert binding.AT3HIP_RESAMPLE_OUT_S16 == 8 == binding.AT3HIP_DECODE_S16 == binding.AT1HIP_DECODE_S16 == binding.AT3PHIP_DECODE_S16


def test_version_stays_1_6():
    assert _lib().at3hip_version() == (1 << 16) | 6
