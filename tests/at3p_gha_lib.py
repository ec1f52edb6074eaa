"""Helpers of the tone-analysis tests (TEST INFRASTRUCTURE: nothing under atracdenc_amd/ imports this module).

  * CpuToneAnalyser: the C restatement tests/host/at3p_gha_cpu.c (include/at3phip.h, FINDING TONES, steps 1-8), compiled on first
    use with the reference's arithmetic flags; one stream, state carried across calls.
  * block_dict / rec_ints: a record of binding.AT3P_TONAL_BLOCK_DTYPE in the dict form of at3p_tonal_lib's restated writer and in
    the flat form at3pt_apply_filter takes.
  * pipeline: the frames at3phip_encode_frames_tonal must write: oracle PQF, the restatement, the division by 32768 / 1.122018,
    oracle MDCT and writer, the block spliced in at the tonal flag.
"""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

from at3_testlib import _vp, at3p_mdct, at3p_pqf, at3p_signal, at3p_write_frames
from at3p_decode_lib import CFLAGS, DELAY
from at3p_tonal_lib import REC_INTS, splice_tonal, tonal_bits

HERE = os.path.dirname(os.path.abspath(__file__))
GHA_SRC = os.path.join(HERE, "host", "at3p_gha_cpu.c")
BLOCK_DTYPE = np.dtype([("num_tone_bands", "u1"), ("second_is_leader", "u1"), ("tone_sharing", "<u2"),
                        ("band", [("n_waves", "u1"), ("start", "u1"), ("stop", "u1"), ("reserved", "u1")], (2, 16)), ("wave", "<u4", 48)])
FIND_TABLES_DTYPE = np.dtype([("sine", "<f4", 2048), ("hann", "<f4", 256), ("amp_sf", "<f4", 64), ("tw", "<f4", 512), ("thr", "<f8", 64), ("rs", "<f8", 1024), ("rc", "<f8", 1024)])
SCALE = 32768.0 / 1.122018
NEW_SYMBOLS = ("at3phip_analyse_tones", "at3phip_encode_frames_tonal", "at3phip_encode_frames_tonal_short", "at3phip_host_tone_find_tables")

_so = None


def gha_lib():
    global _so
    if _so is None:
        d = tempfile.mkdtemp(prefix="at3pgha_")
        so = os.path.join(d, "libat3pgha_cpu.so")
        subprocess.check_call(["gcc", "-std=gnu11", *CFLAGS, "-shared", "-o", so, GHA_SRC, "-lm"])
        _so = so
    lib = ctypes.CDLL(_so)
    lib.at3pg_state_bytes.restype = ctypes.c_size_t
    lib.at3pg_reset.argtypes = [ctypes.c_void_p]
    lib.at3pg_analyse.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.at3pg_tables.argtypes = [ctypes.c_void_p] * 7
    lib.at3pt_filter_bytes.restype = ctypes.c_size_t
    lib.at3pt_apply_filter.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    return lib


class CpuToneAnalyser:
    """One stream of the restatement: analyse(bands [n][C][16][128]) -> (blocks [n], residual [n][C][16][128]) as
    at3phip_analyse_tones returns them for that stream."""

    def __init__(self, channels):
        self.lib = gha_lib()
        self.channels = int(channels)
        self.state = np.zeros(self.lib.at3pg_state_bytes(), np.uint8)
        self.lib.at3pg_reset(_vp(self.state))

    def analyse(self, bands):
        bands = np.ascontiguousarray(bands, np.float32)
        n = bands.shape[0]
        assert bands.shape == (n, self.channels, 16, 128), bands.shape
        blocks = np.zeros(n, BLOCK_DTYPE)
        resid = np.zeros_like(bands)
        self.lib.at3pg_analyse(_vp(self.state), self.channels, _vp(bands), n, _vp(blocks), _vp(resid))
        return blocks, resid


def find_tables():
    t = np.zeros((), FIND_TABLES_DTYPE)
    gha_lib().at3pg_tables(*(_vp(t[k]) for k in ("sine", "hann", "amp_sf", "tw", "thr", "rs", "rc")))
    return t


def band_waves(rec, channels):
    """[ch][16] lists of (FreqIndex, AmpSf, PhaseIndex) of a record"""
    out, at = [], 0
    for ch in range(channels):
        row = []
        for b in range(16):
            n = int(rec["band"][ch, b]["n_waves"])
            row.append([(int(w) & 1023, (int(w) >> 10) & 63, (int(w) >> 16) & 31) for w in rec["wave"][at:at + n]])
            at += n
        out.append(row)
    return out


def n_waves(rec):
    return int(rec["band"]["n_waves"].sum())


def block_dict(rec, channels):
    """the record in the dict form of at3p_tonal_lib.tonal_bits, None for a record without a block"""
    nb = int(rec["num_tone_bands"])
    if nb == 0:
        return None
    waves = band_waves(rec, channels)
    return {"nb": nb, "shared": [False] * nb, "leader": False,
            "bands": [[{"start": None, "stop": None, "waves": waves[ch][b]} for b in range(nb)] for ch in range(channels)]}


def rec_ints(rec, channels):
    """the record in at3pt_apply_filter's flat form (at3pt_unpack_frame's: absent points are start -1, stop 32)"""
    out = np.zeros(REC_INTS, np.int32)
    out[0] = int(rec["num_tone_bands"]) != 0
    waves = band_waves(rec, channels)
    at = 0
    for ch in range(2):
        for b in range(16):
            wv = waves[ch][b] if ch < channels else []
            out[1 + (ch * 16 + b) * 6:1 + (ch * 16 + b) * 6 + 6] = [len(wv), at, 0, -1, 0, 32]
            for fq, sf, ph in wv:
                out[193 + at], out[193 + 48 + at], out[193 + 96 + at] = fq, sf, ph
                at += 1
    return out


def signal_pcm(name, n_frames, channels, scale=1.0):
    """[n_frames][2048][C] of at3p_signal"""
    return np.ascontiguousarray(np.stack([at3p_signal(name, n_frames, channel=c, scale=scale) for c in range(channels)], axis=-1))


def pqf_bands(pcm):
    """pcm [n][2048][C] -> oracle subbands [n][C][16][128]"""
    return np.ascontiguousarray(np.stack([at3p_pqf(np.ascontiguousarray(pcm[:, :, c])) for c in range(pcm.shape[2])], axis=1))


def residual_specs(resid):
    """residual [n][C][16][128] -> spectra [n][C][2048]: the division by 32768 / 1.122018 and the oracle MDCT with sine windows"""
    b = (resid.astype(np.float64) / SCALE).astype(np.float32)
    return np.stack([at3p_mdct(np.ascontiguousarray(b[:, c])) for c in range(resid.shape[1])], axis=1)


def write_residual(resid):
    """residual [n][C][16][128] -> the frames of the oracle writer, without a block"""
    return at3p_write_frames(residual_specs(resid))


def splice_blocks(base, blocks, channels):
    """frame f of base with record blocks[f] spliced in (None / no block: the frame as it is); a block that does not fit is an error"""
    out = []
    for fr, rec in zip(base, blocks):
        b = None if rec is None else block_dict(rec, channels)
        if b is not None:
            fr = splice_tonal(fr, tonal_bits(channels, b))
            assert fr is not None, "the tonal block does not fit the frame"
        out.append(fr)
    return np.stack(out)


def writer_records(blocks):
    """the records the writer pairs with the residual slots: slot f gets the block of slot f - 1, slot 0 none (start of stream)"""
    recs = np.zeros(len(blocks), BLOCK_DTYPE)
    recs[1:] = blocks[:-1]
    return recs


def pipeline(pcm, write=None):
    """pcm [n][2048][C] of one stream from its start -> (frames [n][2048], blocks [n], residual [n][C][16][128]) as
    at3phip_encode_frames_tonal / at3phip_analyse_tones give them: frame f holds residual slot f and the block of slot f - 1.
    write(specs [n][C][2048], records [n]) is the frame writer: by default the oracle's with the block spliced in at the tonal flag,
    which holds where the block leaves the frame its quant units (mono, or quiet stereo); a loud stereo frame needs a writer that
    prices the block (at3phip_write_frames_tonal, pinned to the reference by its own tests)."""
    C = pcm.shape[2]
    blocks, resid = CpuToneAnalyser(C).analyse(pqf_bands(pcm))
    specs, recs = residual_specs(resid), writer_records(blocks)
    frames = write(specs, recs) if write else splice_blocks(at3p_write_frames(specs), recs, C)
    return frames, blocks, resid


BUDGET_FREQS, BUDGET_AMPS = (96, 400, 808), (3000.0, 2750.0, 2500.0)   # close enough for all three to pass the floor of step 3


def budget_bands():
    """[2][2][16][128]: two stereo frames with the same three strong sines in each of the 16 subbands of both channels, continuous
    across the frames: 96 waves are found in the pair, 32 of equal A2 for each sine"""
    t = np.arange(256)
    x = sum(a * np.sin(2 * np.pi * f * (t - 128) / 2048 + 0.3) for f, a in zip(BUDGET_FREQS, BUDGET_AMPS)).astype(np.float32)
    bands = np.zeros((2, 2, 16, 128), np.float32)
    bands[0], bands[1] = x[:128], x[128:]
    return bands


END_FREQS = (1, 2, 5, 9, 1015, 1019, 1022, 1023)


def end_sine_bands():
    """[3][2][16][128]: three stereo frames, subband b of channel c holding a stationary sine at frequency index
    END_FREQS[(b + 3 c) % 8], next to index 0 or 1024, where step 3's end bins and the normalisers of steps 4 and 5 decide"""
    t = np.arange(384)
    bands = np.zeros((3, 2, 16, 128), np.float32)
    for c in range(2):
        for b in range(16):
            f = END_FREQS[(b + 3 * c) % 8]
            bands[:, c, b] = ((300.0 + 40 * b) * np.sin(2 * np.pi * f * t / 2048 + 0.4 * b + c)).astype(np.float32).reshape(3, 128)
    return bands


def snr_db(x, y, n_frames):
    """x the input, y the decoder's output (one channel each, flat): SNR at the codec delay without the first and last two frames"""
    ref = x[2 * 2048:(n_frames - 2) * 2048].astype(np.float64)
    out = y[DELAY + 2 * 2048:DELAY + (n_frames - 2) * 2048].astype(np.float64)
    return 10 * np.log10(np.sum(ref ** 2) / np.sum((ref - out) ** 2))


def export_shim_cases(path, lib_path=None, n=8):
    """tests/host/test_host_shim_at3p_gha.cpp's input: int32 n_cases, then per case int32 channels, frames, the PCM, the oracle's
    subband samples, the restatement's records and residuals, and its pipeline's frames (the writer: at3phip_write_frames_tonal of
    the library at lib_path - the host-compiled kernels, or by default libat3hip.so on a GPU -, which prices the block)"""
    from atracdenc_amd.binding import At3pHip
    with open(path, "wb") as f:
        np.array([2], np.int32).tofile(f)
        for nch, name in ((1, "tones"), (2, "burst")):
            pcm = signal_pcm(name, n, nch)
            enc = At3pHip(n_streams=1, max_frames=n, channels=nch, lib_path=lib_path)
            try:
                frames, blocks, resid = pipeline(pcm, lambda specs, recs: enc.write_frames(specs[None], None, recs[None])[0])
            finally:
                enc.close()
            assert sum(n_waves(b) for b in blocks) > 0
            np.array([nch, n], np.int32).tofile(f)
            for a in (pcm, pqf_bands(pcm), blocks, resid, frames):
                np.ascontiguousarray(a).tofile(f)
    return n
