"""Helpers of the gated tone-analysis tests (TEST INFRASTRUCTURE: nothing under atracdenc_amd/ imports this module).

  * CpuGatedAnalyser: the C restatement tests/host/at3p_gha_gate_cpu.c (include/at3phip.h, FINDING TONES, GATES G1-G5), compiled on
    first use with the reference's arithmetic flags; one stream, state carried across calls; cpu_gates: its G1 alone.
  * block_dict / rec_ints / splice_blocks / pipeline: at3p_gha_lib's, with the records' envelope points.
  * onset_bands / offset_bands: the crafted subband input of the issue's detection cases; keyed_pcm: the `keyed` signal.
"""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

import at3p_gha_lib as G
from at3_testlib import _vp, at3p_write_frames
from at3p_decode_lib import CFLAGS
from at3p_tonal_lib import REC_INTS, splice_tonal, tonal_bits

HERE = os.path.dirname(os.path.abspath(__file__))
GATE_SRC = os.path.join(HERE, "host", "at3p_gha_gate_cpu.c")
GATED = 32   # AT3PHIP_TONES_GATED
GATE_BANDS = (0, 7, 15)
GATE_FREQ, GATE_AMP = 300, 1000.0

_so = {}


def gate_lib(ratio=None):
    """the restatement; ratio: compiled with another R than the header's (the measurement that chose it)"""
    if ratio not in _so:
        d = tempfile.mkdtemp(prefix="at3pgate_")
        so = os.path.join(d, "libat3pgate_cpu.so")
        extra = [] if ratio is None else [f"-DAT3PG_GATE_RATIO={float(ratio)}"]
        subprocess.check_call(["gcc", "-std=gnu11", *CFLAGS, *extra, "-shared", "-o", so, GATE_SRC, "-lm"])
        _so[ratio] = so
    lib = ctypes.CDLL(_so[ratio])
    lib.at3pgg_state_bytes.restype = ctypes.c_size_t
    lib.at3pgg_reset.argtypes = [ctypes.c_void_p]
    lib.at3pgg_analyse.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.at3pg_analyse.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.at3pgg_gates.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.at3pgg_decoder_intervals.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    return lib


class CpuGatedAnalyser:
    """One stream of the restatement: analyse(bands [n][C][16][128]) -> (blocks [n], residual [n][C][16][128]) as
    at3phip_analyse_tones returns them for that stream with AT3PHIP_TONES_GATED (gated=False: without it). `intervals`
    [n][C][16][2] holds the last call's cells [lo, hi] of G3."""

    def __init__(self, channels, gated=True, ratio=None):
        self.lib = gate_lib(ratio)
        self.channels, self.gated = int(channels), bool(gated)
        self.state = np.zeros(self.lib.at3pgg_state_bytes(), np.uint8)
        self.lib.at3pgg_reset(_vp(self.state))
        self.intervals = None

    def analyse(self, bands):
        bands = np.ascontiguousarray(bands, np.float32)
        n = bands.shape[0]
        assert bands.shape == (n, self.channels, 16, 128), bands.shape
        blocks = np.zeros(n, G.BLOCK_DTYPE)
        resid = np.zeros_like(bands)
        if self.gated:
            self.intervals = np.zeros((n, self.channels, 16, 2), np.int8)
            self.lib.at3pgg_analyse(_vp(self.state), self.channels, _vp(bands), n, _vp(blocks), _vp(resid), _vp(self.intervals))
        else:
            self.lib.at3pg_analyse(_vp(self.state), self.channels, _vp(bands), n, _vp(blocks), _vp(resid))
        return blocks, resid


def cpu_gates(bands, ratio=None):
    """bands [n][C][16][128] -> [n][C][16] bytes of G1"""
    bands = np.ascontiguousarray(bands, np.float32)
    out = np.zeros(bands.shape[:3], np.uint8)
    gate_lib(ratio).at3pgg_gates(_vp(bands), bands.shape[0], bands.shape[1], _vp(out))
    return out


def decoder_intervals(rec, channels):
    """unpacked records [n][REC_INTS] (at3p_tonal_lib.unpack_tonal) of consecutive frames -> [n][C][16][2]: the cells [lo, hi]
    of the curr_env the restated decoder reconstructs for each"""
    rec = np.ascontiguousarray(rec, np.int32)
    out = np.zeros((rec.shape[0], channels, 16, 2), np.int8)
    gate_lib().at3pgg_decoder_intervals(channels, _vp(rec), REC_INTS, rec.shape[0], _vp(out))
    return out


def points(rec, channels):
    """{(ch, band): (start, stop)} of the record's points, in the record's "+1" convention, absent points left out"""
    return {(ch, b): (int(rec["band"][ch, b]["start"]), int(rec["band"][ch, b]["stop"]))
            for ch in range(channels) for b in range(16) if rec["band"][ch, b]["start"] or rec["band"][ch, b]["stop"]}


def block_dict(rec, channels):
    """the record in the dict form of at3p_tonal_lib.tonal_bits, points included; None for a record without a block"""
    d = G.block_dict(rec, channels)
    if d is not None:
        for ch in range(channels):
            for b in range(d["nb"]):
                st, sp = int(rec["band"][ch, b]["start"]), int(rec["band"][ch, b]["stop"])
                d["bands"][ch][b]["start"], d["bands"][ch][b]["stop"] = (st - 1 if st else None), (sp - 1 if sp else None)
    return d


def rec_ints(rec, channels):
    """the record in at3pt_apply_filter's flat form, points included"""
    out = G.rec_ints(rec, channels)
    for ch in range(channels):
        for b in range(16):
            st, sp = int(rec["band"][ch, b]["start"]), int(rec["band"][ch, b]["stop"])
            at = 1 + (ch * 16 + b) * 6
            if st:
                out[at + 2], out[at + 3] = 1, st - 1
            if sp:
                out[at + 4], out[at + 5] = 1, sp - 1
    return out


def splice_blocks(base, blocks, channels):
    """at3p_gha_lib.splice_blocks with the points written"""
    out = []
    for fr, rec in zip(base, blocks):
        b = None if rec is None else block_dict(rec, channels)
        if b is not None:
            fr = splice_tonal(fr, tonal_bits(channels, b))
            assert fr is not None, "the tonal block does not fit the frame"
        out.append(fr)
    return np.stack(out)


def pipeline(pcm, gated=True, write=None, ratio=None):
    """at3p_gha_lib.pipeline with the gated restatement: the frames at3phip_encode_frames_tonal must write with
    AT3PHIP_TONES_GATED"""
    C = pcm.shape[2]
    blocks, resid = CpuGatedAnalyser(C, gated, ratio).analyse(G.pqf_bands(pcm))
    specs, recs = G.residual_specs(resid), G.writer_records(blocks)
    frames = write(specs, recs) if write else splice_blocks(at3p_write_frames(specs), recs, C)
    return frames, blocks, resid


def _gate_sine(n_frames):
    t = np.arange(128 * n_frames)
    return (GATE_AMP * np.sin(2 * np.pi * GATE_FREQ * t / 2048 + 0.7)).astype(np.float32)


def onset_bands(s0, channels, n_frames=6, frame=2):
    """[n_frames][C][16][128]: subbands 0, 7 and 15 of every channel hold a sine at frequency index 300 that is exactly zero before
    cell s0 of frame `frame` and continuous afterwards; every other subband is zero"""
    x = _gate_sine(n_frames)
    x[:128 * frame + 4 * s0] = 0.0
    bands = np.zeros((n_frames, channels, 16, 128), np.float32)
    for b in GATE_BANDS:
        bands[:, :, b] = x.reshape(n_frames, 1, 128)
    return bands


def offset_bands(p0, channels, n_frames=6, frame=2):
    """the mirrored signal: the same sine from the stream's start, switched off after cell p0 of frame `frame`"""
    x = _gate_sine(n_frames)
    x[128 * frame + 4 * (p0 + 1):] = 0.0
    bands = np.zeros((n_frames, channels, 16, 128), np.float32)
    for b in GATE_BANDS:
        bands[:, :, b] = x.reshape(n_frames, 1, 128)
    return bands


def crafted_cases(channels):
    """{name: bands [6][C][16][128]}: the issue's onsets at cells 4, 16, 28 and the mirrored offsets after cells 3, 15, 27"""
    out = {f"onset{s0}": onset_bands(s0, channels) for s0 in (4, 16, 28)}
    out.update({f"offset{p0}": offset_bands(p0, channels) for p0 in (3, 15, 27)})
    return out


def export_shim_cases(path, lib_path=None, n=8):
    """tests/host/test_host_shim_at3p_gha_gate.cpp's input: int32 n_cases, then per case int32 channels, frames, with_pcm, the PCM
    (with_pcm only), the subband samples, the gated restatement's records and residuals, and (with_pcm only) its pipeline's
    frames (the writer: at3phip_write_frames_tonal of the library at lib_path, which prices the block). Returns
    [(channels, frames, with_pcm)]."""
    from atracdenc_amd.binding import At3pHip
    cases = []
    for nch, name in ((1, "keyed"), (2, "burst")):
        pcm = keyed_pcm(n, nch) if name == "keyed" else G.signal_pcm(name, n, nch)
        enc = At3pHip(n_streams=1, max_frames=n, channels=nch, lib_path=lib_path)
        try:
            frames, blocks, resid = pipeline(pcm, True, lambda specs, recs: enc.write_frames(specs[None], None, recs[None])[0])
        finally:
            enc.close()
        assert sum(len(points(b, nch)) for b in blocks) > 0 and sum(G.n_waves(b) for b in blocks) > 0
        cases.append((nch, n, 1, pcm, G.pqf_bands(pcm), blocks, resid, frames))
    for nch, name in ((2, "onset16"), (1, "offset15"), (2, "onset28"), (1, "offset3")):
        bands = crafted_cases(nch)[name]
        blocks, resid = CpuGatedAnalyser(nch).analyse(bands)
        cases.append((nch, bands.shape[0], 0, None, bands, blocks, resid, None))
    with open(path, "wb") as f:
        np.array([len(cases)], np.int32).tofile(f)
        for nch, nf, with_pcm, *arrays in cases:
            np.array([nch, nf, with_pcm], np.int32).tofile(f)
            for a in arrays:
                if a is not None:
                    np.ascontiguousarray(a).tofile(f)
    return [c[:3] for c in cases]


def onset_pcm(n_frames, channels, at=2 * 2048 + 1000):
    """[n_frames][2048][C]: a 3 kHz sine at 0.5 that is exactly zero before sample `at` and continuous afterwards"""
    t = np.arange(n_frames * 2048)
    x = (0.5 * np.sin(2 * np.pi * 3000.0 * t / 44100.0) * (t >= at)).astype(np.float32)
    return np.ascontiguousarray(np.repeat(x.reshape(n_frames, 2048, 1), channels, axis=2))


def keyed_pcm(n_frames, channels):
    """[n_frames][2048][C]: `keyed`, a 3 kHz sine at 0.5, fully on and off every 3000 samples"""
    t = np.arange(n_frames * 2048)
    x = (0.5 * np.sin(2 * np.pi * 3000.0 * t / 44100.0) * ((t // 3000) % 2 == 0)).astype(np.float32)
    return np.ascontiguousarray(np.repeat(x.reshape(n_frames, 2048, 1), channels, axis=2))
