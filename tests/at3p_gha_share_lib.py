"""Helpers of the shared-band tone-analysis tests (TEST INFRASTRUCTURE: nothing under atracdenc_amd/ imports this module).

  * CpuSharedAnalyser: the C restatement tests/host/at3p_gha_share_cpu.c (include/at3phip.h, FINDING TONES, SHARING S1-S5), compiled
    on first use with the reference's arithmetic flags; one stream, state carried across calls, any combination of
    AT3PHIP_TONES_GATED and AT3PHIP_TONES_SHARED.
  * block_dict / rec_ints / splice_blocks / pipeline: at3p_gha_gate_lib's, with the records' sharing word.
  * the crafted input of the issue's cases: budget (every band a twin), differ (band 5 of channel 1 differs), onset_both and
    onset_one (gates), dense_pcm (the round trip's signal).
"""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

import at3p_gha_gate_lib as GG
import at3p_gha_lib as G
from at3_testlib import _vp, at3p_write_frames
from at3p_decode_lib import CFLAGS
from at3p_tonal_lib import splice_tonal, tonal_bits

HERE = os.path.dirname(os.path.abspath(__file__))
SHARE_SRC = os.path.join(HERE, "host", "at3p_gha_share_cpu.c")
GATED, SHARED = 32, 64   # AT3PHIP_TONES_GATED, AT3PHIP_TONES_SHARED
DIFFER_BAND, DIFFER_AMP = 5, 3750.0   # case 2: the sine at index 808 of channel 1's band 5, 2500 -> 3750: 4 log2(1.5) = 2.3 AmpSf steps

_so = None


def share_lib():
    global _so
    if _so is None:
        d = tempfile.mkdtemp(prefix="at3pshare_")
        so = os.path.join(d, "libat3pshare_cpu.so")
        subprocess.check_call(["gcc", "-std=gnu11", *CFLAGS, "-shared", "-o", so, SHARE_SRC, "-lm"])
        _so = so
    lib = ctypes.CDLL(_so)
    lib.at3pgs_state_bytes.restype = ctypes.c_size_t
    lib.at3pgs_reset.argtypes = [ctypes.c_void_p]
    lib.at3pgs_analyse.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
    return lib


def flags(gated, shared):
    return (GATED if gated else 0) | (SHARED if shared else 0)


class CpuSharedAnalyser:
    """One stream of the restatement: analyse(bands [n][C][16][128]) -> (blocks [n], residual [n][C][16][128]) as
    at3phip_analyse_tones returns them for that stream with the given flags. `found` [n] holds the last call's wave counts
    before the budget."""

    def __init__(self, channels, gated=False, shared=True):
        self.lib = share_lib()
        self.channels, self.flags = int(channels), flags(gated, shared)
        self.state = np.zeros(self.lib.at3pgs_state_bytes(), np.uint8)
        self.lib.at3pgs_reset(_vp(self.state))
        self.found = None

    def analyse(self, bands):
        bands = np.ascontiguousarray(bands, np.float32)
        n = bands.shape[0]
        assert bands.shape == (n, self.channels, 16, 128), bands.shape
        blocks = np.zeros(n, G.BLOCK_DTYPE)
        resid = np.zeros_like(bands)
        self.found = np.zeros(n, np.int32)
        self.lib.at3pgs_analyse(_vp(self.state), self.channels, _vp(bands), n, _vp(blocks), _vp(resid), self.flags, _vp(self.found))
        return blocks, resid


def shared_bands(rec):
    """the bands whose sharing bit is set"""
    return [b for b in range(16) if (int(rec["tone_sharing"]) >> b) & 1]


def block_dict(rec, channels):
    """the record in the dict form of at3p_tonal_lib.tonal_bits, points and sharing flags included; None without a block"""
    d = GG.block_dict(rec, channels)
    if d is not None:
        d["shared"] = [bool((int(rec["tone_sharing"]) >> b) & 1) for b in range(d["nb"])]
    return d


def block_bits(rec, channels):
    """the length of the record's tonal block in bits, as the restated writer writes it (0 without a block)"""
    d = block_dict(rec, channels)
    return 0 if d is None else sum(n for _, n in tonal_bits(channels, d))


def rec_ints(rec, channels):
    """the record in at3pt_apply_filter's flat form, as the decoder holds it after its copy of the shared bands"""
    out = GG.rec_ints(rec, channels)
    for b in shared_bands(rec):
        if b < int(rec["num_tone_bands"]):
            out[1 + (16 + b) * 6:1 + (16 + b) * 6 + 6] = out[1 + b * 6:1 + b * 6 + 6]
    return out


def splice_blocks(base, blocks, channels):
    """at3p_gha_lib.splice_blocks with the points and the sharing flags written"""
    out = []
    for fr, rec in zip(base, blocks):
        b = None if rec is None else block_dict(rec, channels)
        if b is not None:
            fr = splice_tonal(fr, tonal_bits(channels, b))
            assert fr is not None, "the tonal block does not fit the frame"
        out.append(fr)
    return np.stack(out)


def pipeline(pcm, gated=False, shared=True, write=None):
    """at3p_gha_lib.pipeline with this restatement: the frames at3phip_encode_frames_tonal must write with the given flags"""
    C = pcm.shape[2]
    blocks, resid = CpuSharedAnalyser(C, gated, shared).analyse(G.pqf_bands(pcm))
    specs, recs = G.residual_specs(resid), G.writer_records(blocks)
    frames = write(specs, recs) if write else splice_blocks(at3p_write_frames(specs), recs, C)
    return frames, blocks, resid


def budget_bands(n=2, differ=False):
    """[n][2][16][128]: G.budget_bands() continued over n frames (the same three sines in all 16 subbands of both channels);
    differ: the sine at index 808 of channel 1's band DIFFER_BAND has amplitude DIFFER_AMP instead of 2500"""
    t = np.arange(128 * n)

    def x(amps):
        return sum(a * np.sin(2 * np.pi * f * (t - 128) / 2048 + 0.3) for f, a in zip(G.BUDGET_FREQS, amps)).astype(np.float32).reshape(n, 128)

    bands = np.zeros((n, 2, 16, 128), np.float32)
    bands[:] = x(G.BUDGET_AMPS)[:, None, None, :]
    if differ:
        bands[:, 1, DIFFER_BAND] = x(G.BUDGET_AMPS[:2] + (DIFFER_AMP,))
    return bands


def onset_bands(both, n=6, s0=16):
    """[n][2][16][128]: GG.onset_bands (an onset at cell s0 of frame 2 in bands 0, 7 and 15); both: in both channels alike; else
    in channel 1 only, channel 0 holding the same sine from the stream's start"""
    bands = GG.onset_bands(s0, 2, n)
    if not both:
        steady = GG._gate_sine(n).reshape(n, 128)
        for b in GG.GATE_BANDS:
            bands[:, 0, b] = steady
    return bands


CASES = {   # name: (bands [n][2][16][128] for n frames, gated)
    "budget": (lambda n: budget_bands(n), False),
    "differ": (lambda n: budget_bands(n, True), False),
    "onset_both": (lambda n: onset_bands(True, n), True),
    "onset_one": (lambda n: onset_bands(False, n), True),
}


def dense_pcm(n_frames, subbands=10, amp=0.02):
    """[n_frames][2048][2], both channels alike: three sines in each of subbands 1 .. `subbands`, sine j = 0..2 of subband b at
    (b + (j + 1) / 4) * 22050 / 16 Hz with amplitude `amp` and phase 0.37 k for the k-th sine"""
    t = np.arange(n_frames * 2048, dtype=np.float64)
    x = np.zeros(n_frames * 2048)
    k = 0
    for b in range(1, subbands + 1):
        for j in range(3):
            x += amp * np.sin(2 * np.pi * (b + (j + 1) / 4.0) * 22050.0 / 16.0 * t / 44100.0 + 0.37 * k)
            k += 1
    return np.ascontiguousarray(np.repeat(x.astype(np.float32).reshape(n_frames, 2048, 1), 2, axis=2))


def twin_pcm(name, n_frames, scale=1.0):
    """[n_frames][2048][2]: channel 0 of at3p_signal in both channels"""
    return np.ascontiguousarray(np.repeat(G.signal_pcm(name, n_frames, 1, scale), 2, axis=2))


def export_shim_cases(path, lib_path=None, n=8):
    """tests/host/test_host_shim_at3p_share.cpp's input: int32 n_cases, then per case int32 channels, frames, flags, with_pcm, the PCM
    (with_pcm only), the subband samples, the restatement's records and residuals, and (with_pcm only) its pipeline's frames (the
    writer: at3phip_write_frames_tonal of the library at lib_path, which prices the block). Returns [(channels, frames, flags,
    with_pcm)]."""
    from atracdenc_amd.binding import At3pHip
    cases = []
    for name, nch, gated in (("tones", 2, False), ("burst", 2, True), ("tones", 1, False)):
        pcm = twin_pcm(name, n) if nch == 2 else G.signal_pcm(name, n, 1)
        enc = At3pHip(n_streams=1, max_frames=n, channels=nch, lib_path=lib_path)
        try:
            frames, blocks, resid = pipeline(pcm, gated, True, lambda specs, recs: enc.write_frames(specs[None], None, recs[None])[0])
        finally:
            enc.close()
        assert sum(G.n_waves(b) for b in blocks) > 0 and (nch == 1 or sum(len(shared_bands(b)) for b in blocks) > 0)
        cases.append((nch, n, flags(gated, True), 1, pcm, G.pqf_bands(pcm), blocks, resid, frames))
    for name, (make, gated) in CASES.items():
        bands = make(6)
        blocks, resid = CpuSharedAnalyser(2, gated, True).analyse(bands)
        cases.append((2, bands.shape[0], flags(gated, True), 0, None, bands, blocks, resid, None))
    with open(path, "wb") as f:
        np.array([len(cases)], np.int32).tofile(f)
        for nch, nf, fl, with_pcm, *arrays in cases:
            np.array([nch, nf, fl, with_pcm], np.int32).tofile(f)
            for a in arrays:
                if a is not None:
                    np.ascontiguousarray(a).tofile(f)
    return [c[:4] for c in cases]
