"""Helpers of the tone-analysis tests (TEST INFRASTRUCTURE: nothing under atracdenc_amd/ imports this module).

  * CpuToneAnalyser: the C restatement tests/host/at3p_gha_cpu.c (include/at3phip.h, FINDING TONES: steps 1-8, GATES G1-G5, SHARING
    S1-S5), compiled on first use with the reference's arithmetic flags; one stream, state carried across calls, any combination of
    AT3PHIP_TONES_GATED and AT3PHIP_TONES_SHARED; cpu_gates: its G1 alone.
  * block_dict / rec_ints: a record of binding.AT3P_TONAL_BLOCK_DTYPE in the dict form of at3p_tonal_lib's restated writer and in
    the flat form at3pt_apply_filter takes, envelope points and sharing flags included.
  * pipeline: the frames at3phip_encode_frames_tonal must write: oracle PQF, the restatement, the division by 32768 / 1.122018,
    oracle MDCT and writer, the block spliced in at the tonal flag.
  * the crafted input of the tests: budget_bands (every band a twin; differ: band 5 of channel 1 differs), end_sine_bands,
    onset_bands / offset_bands / crafted_cases (gates), stereo_onset_bands and CASES (gates with sharing), keyed_pcm, onset_pcm,
    dense_pcm, twin_pcm.
  * export_shim_cases: the input of tests/host/test_host_shim_at3p_gha.cpp; flag_digests: tests/golden/at3p_gha_flags.npz.
"""
import ctypes
import functools
import hashlib
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
GATED, SHARED = 32, 64   # AT3PHIP_TONES_GATED, AT3PHIP_TONES_SHARED
GATE_BANDS = (0, 7, 15)
GATE_FREQ, GATE_AMP = 300, 1000.0
DIFFER_BAND, DIFFER_AMP = 5, 3750.0   # the sine at index 808 of channel 1's band 5, 2500 -> 3750: 4 log2(1.5) = 2.3 AmpSf steps
NEW_SYMBOLS = ("at3phip_analyse_tones", "at3phip_encode_frames_tonal", "at3phip_encode_frames_tonal_short", "at3phip_host_tone_find_tables")

_so = {}


def gha_lib(ratio=None):
    """the restatement; ratio: compiled with another R than the header's (the measurement that chose it)"""
    if ratio not in _so:
        d = tempfile.mkdtemp(prefix="at3pgha_")
        so = os.path.join(d, "libat3pgha_cpu.so")
        extra = [] if ratio is None else [f"-DAT3PG_GATE_RATIO={float(ratio)}"]
        subprocess.check_call(["gcc", "-std=gnu11", *CFLAGS, *extra, "-shared", "-o", so, GHA_SRC, "-lm"])
        _so[ratio] = so
    lib = ctypes.CDLL(_so[ratio])
    lib.at3pg_state_bytes.restype = ctypes.c_size_t
    lib.at3pg_reset.argtypes = [ctypes.c_void_p]
    lib.at3pg_analyse.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
                                  ctypes.c_void_p, ctypes.c_void_p]
    lib.at3pg_tables.argtypes = [ctypes.c_void_p] * 7
    lib.at3pg_gates.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.at3pg_decoder_intervals.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.at3pt_filter_bytes.restype = ctypes.c_size_t
    lib.at3pt_apply_filter.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def flags(gated, shared):
    return (GATED if gated else 0) | (SHARED if shared else 0)


class CpuToneAnalyser:
    """One stream of the restatement: analyse(bands [n][C][16][128]) -> (blocks [n], residual [n][C][16][128]) as
    at3phip_analyse_tones returns them for that stream with the given flags. Of the last call, `intervals` [n][C][16][2] holds
    the cells [lo, hi] of G3 and `found` [n] the wave counts before the budget."""

    def __init__(self, channels, gated=False, shared=False, ratio=None):
        self.lib = gha_lib(ratio)
        self.channels, self.flags = int(channels), flags(gated, shared)
        self.state = np.zeros(self.lib.at3pg_state_bytes(), np.uint8)
        self.lib.at3pg_reset(_vp(self.state))
        self.intervals = self.found = None

    def analyse(self, bands):
        bands = np.ascontiguousarray(bands, np.float32)
        n = bands.shape[0]
        assert bands.shape == (n, self.channels, 16, 128), bands.shape
        blocks = np.zeros(n, BLOCK_DTYPE)
        resid = np.zeros_like(bands)
        self.intervals, self.found = np.zeros((n, self.channels, 16, 2), np.int8), np.zeros(n, np.int32)
        self.lib.at3pg_analyse(_vp(self.state), self.channels, _vp(bands), n, _vp(blocks), _vp(resid), self.flags, _vp(self.intervals), _vp(self.found))
        return blocks, resid


def cpu_gates(bands, ratio=None):
    """bands [n][C][16][128] -> [n][C][16] bytes of G1"""
    bands = np.ascontiguousarray(bands, np.float32)
    out = np.zeros(bands.shape[:3], np.uint8)
    gha_lib(ratio).at3pg_gates(_vp(bands), bands.shape[0], bands.shape[1], _vp(out))
    return out


def decoder_intervals(rec, channels):
    """unpacked records [n][REC_INTS] (at3p_tonal_lib.unpack_tonal) of consecutive frames -> [n][C][16][2]: the cells [lo, hi]
    of the curr_env the restated decoder reconstructs for each"""
    rec = np.ascontiguousarray(rec, np.int32)
    out = np.zeros((rec.shape[0], channels, 16, 2), np.int8)
    gha_lib().at3pg_decoder_intervals(channels, _vp(rec), REC_INTS, rec.shape[0], _vp(out))
    return out


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


def points(rec, channels):
    """{(ch, band): (start, stop)} of the record's points, in the record's "+1" convention, absent points left out"""
    return {(ch, b): (int(rec["band"][ch, b]["start"]), int(rec["band"][ch, b]["stop"]))
            for ch in range(channels) for b in range(16) if rec["band"][ch, b]["start"] or rec["band"][ch, b]["stop"]}


def shared_bands(rec):
    """the bands whose sharing bit is set"""
    return [b for b in range(16) if (int(rec["tone_sharing"]) >> b) & 1]


def block_dict(rec, channels):
    """the record in the dict form of at3p_tonal_lib.tonal_bits, points and sharing flags included; None for a record without a
    block"""
    nb = int(rec["num_tone_bands"])
    if nb == 0:
        return None
    waves, pt = band_waves(rec, channels), points(rec, channels)

    def band(ch, b):
        st, sp = pt.get((ch, b), (0, 0))
        return {"start": st - 1 if st else None, "stop": sp - 1 if sp else None, "waves": waves[ch][b]}

    return {"nb": nb, "shared": [b in shared_bands(rec) for b in range(nb)], "leader": False,
            "bands": [[band(ch, b) for b in range(nb)] for ch in range(channels)]}


def block_bits(rec, channels):
    """the length of the record's tonal block in bits, as the restated writer writes it (0 without a block)"""
    d = block_dict(rec, channels)
    return 0 if d is None else sum(n for _, n in tonal_bits(channels, d))


def rec_ints(rec, channels):
    """the record in at3pt_apply_filter's flat form (at3pt_unpack_frame's: absent points are start -1, stop 32), as the decoder
    holds it after its copy of the shared bands"""
    out = np.zeros(REC_INTS, np.int32)
    out[0] = int(rec["num_tone_bands"]) != 0
    waves, pt = band_waves(rec, channels), points(rec, channels)
    at = 0
    for ch in range(2):
        for b in range(16):
            wv = waves[ch][b] if ch < channels else []
            st, sp = pt.get((ch, b), (0, 0))
            out[1 + (ch * 16 + b) * 6:1 + (ch * 16 + b) * 6 + 6] = [len(wv), at, st != 0, st - 1, sp != 0, sp - 1 if sp else 32]
            for fq, sf, ph in wv:
                out[193 + at], out[193 + 48 + at], out[193 + 96 + at] = fq, sf, ph
                at += 1
    for b in shared_bands(rec):
        if b < int(rec["num_tone_bands"]):
            out[1 + (16 + b) * 6:1 + (16 + b) * 6 + 6] = out[1 + b * 6:1 + b * 6 + 6]
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


def pipeline(pcm, gated=False, shared=False, write=None, ratio=None):
    """pcm [n][2048][C] of one stream from its start -> (frames [n][2048], blocks [n], residual [n][C][16][128]) as
    at3phip_encode_frames_tonal / at3phip_analyse_tones give them with the given flags: frame f holds residual slot f and the block
    of slot f - 1. write(specs [n][C][2048], records [n]) is the frame writer: by default the oracle's with the block spliced in at
    the tonal flag, which holds where the block leaves the frame its quant units (mono, or quiet stereo); a loud stereo frame needs
    a writer that prices the block (at3phip_write_frames_tonal, pinned to the reference by its own tests)."""
    C = pcm.shape[2]
    blocks, resid = CpuToneAnalyser(C, gated, shared, ratio).analyse(pqf_bands(pcm))
    specs, recs = residual_specs(resid), writer_records(blocks)
    frames = write(specs, recs) if write else splice_blocks(at3p_write_frames(specs), recs, C)
    return frames, blocks, resid


BUDGET_FREQS, BUDGET_AMPS = (96, 400, 808), (3000.0, 2750.0, 2500.0)   # close enough for all three to pass the floor of step 3


def budget_bands(n=2, differ=False):
    """[n][2][16][128]: n stereo frames with the same three strong sines in each of the 16 subbands of both channels, continuous
    across the frames: 96 waves are found in a pair, 32 of equal A2 for each sine. differ: the sine at index 808 of channel 1's
    band DIFFER_BAND has amplitude DIFFER_AMP instead of 2500"""
    t = np.arange(128 * n)

    def x(amps):
        return sum(a * np.sin(2 * np.pi * f * (t - 128) / 2048 + 0.3) for f, a in zip(BUDGET_FREQS, amps)).astype(np.float32).reshape(n, 128)

    bands = np.zeros((n, 2, 16, 128), np.float32)
    bands[:] = x(BUDGET_AMPS)[:, None, None, :]
    if differ:
        bands[:, 1, DIFFER_BAND] = x(BUDGET_AMPS[:2] + (DIFFER_AMP,))
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


def stereo_onset_bands(both, n=6, s0=16):
    """[n][2][16][128]: onset_bands (an onset at cell s0 of frame 2 in bands 0, 7 and 15); both: in both channels alike; else
    in channel 1 only, channel 0 holding the same sine from the stream's start"""
    bands = onset_bands(s0, 2, n)
    if not both:
        steady = _gate_sine(n).reshape(n, 128)
        for b in GATE_BANDS:
            bands[:, 0, b] = steady
    return bands


CASES = {   # name: (bands [n][2][16][128] for n frames, gated)
    "budget": (lambda n: budget_bands(n), False),
    "differ": (lambda n: budget_bands(n, True), False),
    "onset_both": (lambda n: stereo_onset_bands(True, n), True),
    "onset_one": (lambda n: stereo_onset_bands(False, n), True),
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
    return np.ascontiguousarray(np.repeat(signal_pcm(name, n_frames, 1, scale), 2, axis=2))


SHIM_CRAFTED = ((2, "onset16"), (1, "offset15"), (2, "onset28"), (1, "offset3"))   # the gated shim cases without PCM


def export_shim_cases(path, lib_path=None, which="plain", n=8):
    """tests/host/test_host_shim_at3p_gha.cpp's input: int32 n_cases, then per case int32 channels, frames, flags, with_pcm, the PCM
    (with_pcm only), the subband samples, the restatement's records and residuals under those flags, and (with_pcm only) its
    pipeline's frames (the writer: at3phip_write_frames_tonal of the library at lib_path - the host-compiled kernels, or by default
    libat3hip.so on a GPU -, which prices the block). which: "plain" (mono tones, stereo burst), "gated" (keyed, burst, four crafted
    events) or "shared" (twin tones, twin burst with gates, mono tones, CASES). Returns [(channels, frames, flags, with_pcm)]."""
    from atracdenc_amd.binding import At3pHip
    with_pcm, crafted = {
        "plain": ([(signal_pcm("tones", n, 1), 0), (signal_pcm("burst", n, 2), 0)], []),
        "gated": ([(keyed_pcm(n, 1), GATED), (signal_pcm("burst", n, 2), GATED)], [(crafted_cases(nch)[name], GATED) for nch, name in SHIM_CRAFTED]),
        "shared": ([(twin_pcm("tones", n), SHARED), (twin_pcm("burst", n), GATED | SHARED), (signal_pcm("tones", n, 1), SHARED)],
                   [(make(6), flags(gated, True)) for make, gated in CASES.values()]),
    }[which]
    cases = []
    for pcm, fl in with_pcm:
        nch = pcm.shape[2]
        enc = At3pHip(n_streams=1, max_frames=n, channels=nch, lib_path=lib_path)
        try:
            frames, blocks, resid = pipeline(pcm, fl & GATED, fl & SHARED, lambda specs, recs: enc.write_frames(specs[None], None, recs[None])[0])
        finally:
            enc.close()
        assert sum(n_waves(b) for b in blocks) > 0
        assert not fl & GATED or sum(len(points(b, nch)) for b in blocks) > 0
        assert not fl & SHARED or nch == 1 or sum(len(shared_bands(b)) for b in blocks) > 0
        cases.append((nch, n, fl, 1, pcm, pqf_bands(pcm), blocks, resid, frames))
    for bands, fl in crafted:
        nch = bands.shape[1]
        blocks, resid = CpuToneAnalyser(nch, fl & GATED, fl & SHARED).analyse(bands)
        cases.append((nch, bands.shape[0], fl, 0, None, bands, blocks, resid, None))
    with open(path, "wb") as f:
        np.array([len(cases)], np.int32).tofile(f)
        for *head, pcm, bands, blocks, resid, frames in cases:
            np.array(head, np.int32).tofile(f)
            for a in (pcm, bands, blocks, resid, frames):
                if a is not None:
                    np.ascontiguousarray(a).tofile(f)
    return [tuple(c[:4]) for c in cases]


# ---- tests/golden/at3p_gha_flags.npz: the restatement pinned to what its three layered predecessors computed ------------------------
def digests(blocks, resid):
    """[SHA-256 of the records, SHA-256 of the residuals]"""
    return [hashlib.sha256(blocks.tobytes()).hexdigest(), hashlib.sha256(resid.tobytes()).hexdigest()]


@functools.lru_cache(None)
def flag_digest_cases():
    """[(key, bands, flags)] of the fixture: the key names the entry point whose output was recorded before the restatements were
    merged (pg: at3pg_analyse without flags, pgg: at3pgg_analyse with GATED, pgs: at3pgs_analyse with any flags), the input, its
    channels and the flags. The inputs: the crafted events in mono and stereo, the budget's pair and the stereo onset, unflagged
    and gated as the layered files' own entry points saw them; CASES at 6 frames and the shim's crafted events under every
    combination of the two flags."""
    out = [(f"pg_{name}_{nch}_0", bands, 0) for nch in (1, 2) for name, bands in crafted_cases(nch).items()]
    out.append(("pg_budget_pair_2_0", budget_bands(), 0))
    out.append((f"pgg_onset_both_2_{GATED}", stereo_onset_bands(True), GATED))
    both = [(name, make(6)) for name, (make, _) in CASES.items()] + [(name, crafted_cases(nch)[name]) for nch, name in SHIM_CRAFTED]
    out += [(f"pgs_{name}_{bands.shape[1]}_{fl}", bands, fl) for name, bands in both for fl in (0, GATED, SHARED, GATED | SHARED)]
    return out


_flag_golden = None


def assert_flag_digests(key, bands, got=None):
    """the restatement's records and residuals for the fixture's `key` are the recorded ones; got: (blocks, residual) already
    computed for it, else they are computed here"""
    global _flag_golden
    if _flag_golden is None:
        _flag_golden = np.load(os.path.join(HERE, "golden", "at3p_gha_flags.npz"))
    fl = int(key.rsplit("_", 1)[1])
    blocks, resid = got or CpuToneAnalyser(bands.shape[1], fl & GATED, fl & SHARED).analyse(bands)
    assert digests(blocks, resid) == _flag_golden[key].tolist(), key
