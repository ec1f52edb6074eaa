"""ATRAC3plus rate-distortion and masking-weighted word lengths on the GPU (AT3PHIP_ALLOC_RD, AT3PHIP_ALLOC_PSY; include/at3phip.h,
RATE-DISTORTION WORD LENGTHS and MASKING-WEIGHTED WORD LENGTHS), every test once per mode: the six frame-writing calls with ADAPTIVE |
SPARSE | RD (| PSY) equal the restatement tests/host/at3p_rd_cpu.c byte for byte - host and device buffers, queued and waiting, however
the stream is split, whatever the calls before carried -; non-finite spectra in one stream leave the others alone; the mode's flag
without the flags it needs is refused and moves nothing; the frames decode on the GPU decoder with every counter zero. 3 streams x 3
frames; what does not depend on the frame size (spectra, tone analysis) is computed once."""
import numpy as np
import pytest

import at3p_psy_lib as Y
import at3p_writer_lib as W
import at3p_gha_lib as G
import at3p_tonal_write_lib as TW
from at3_testlib import at3p_mdct, at3p_pqf

pytestmark = pytest.mark.gpu
S, F = 3, 3
SENTINEL = 0xA5
MODES = ("rd", "psy")
# per mode: the binding's keywords; the older mode that "switched between calls" and "frames differ from" compare with; the sizes of the
# writer tests and of the decoder test; the flag's name, every flag set without all it needs, the refusal's text and the keyword sets the
# binding itself refuses
KWS = {"rd": dict(adaptive=True, sparse=True, rd=True), "psy": dict(adaptive=True, sparse=True, rd=True, psy=True)}
OLDER_KW = {"rd": dict(adaptive=True, sparse=True), "psy": dict(adaptive=True, sparse=True, rd=True)}
CASES = {"rd": [(1, 176), (1, 376), (1, 744), (1, 2048), (2, 224), (2, 376), (2, 744), (2, 2048)],
         "psy": [(1, 176), (1, 376), (1, 2048), (2, 224), (2, 376), (2, 2048)]}
DECODE_CASES = {"rd": [(1, 176), (2, 224), (2, 376), (2, 744)], "psy": [(1, 176), (2, 224), (2, 376)]}
DEVICE_CASES = [(1, 176), (2, 376), (2, 2048)]
FLAG = {"rd": "AT3PHIP_ALLOC_RD", "psy": "AT3PHIP_ALLOC_PSY"}
LACKING = {"rd": [(), ("ADAPTIVE",), ("SPARSE",)],
           "psy": [(), ("ADAPTIVE",), ("SPARSE",), ("RD",), ("ADAPTIVE", "SPARSE"), ("ADAPTIVE", "RD"), ("SPARSE", "RD")]}
REFUSAL = {"rd": "AT3PHIP_ALLOC_RD needs AT3PHIP_ALLOC_ADAPTIVE and AT3PHIP_ALLOC_SPARSE",
           "psy": "AT3PHIP_ALLOC_PSY needs AT3PHIP_ALLOC_ADAPTIVE, AT3PHIP_ALLOC_SPARSE and AT3PHIP_ALLOC_RD"}
BAD_KW = {"rd": (dict(rd=True), dict(adaptive=True, rd=True)), "psy": (dict(psy=True), dict(adaptive=True, sparse=True, psy=True))}


def _id(mode, rest):
    """a case's id: rd's are the ids this module had before it took a second mode, psy's carry the mode in front"""
    return rest if mode == "rd" else f"{mode}-{rest}"


def _per_mode(cases):
    """parametrize("mode,nch,fb") over a list of (nch, fb), or one list per mode"""
    rows = [(m, nch, fb) for m in MODES for nch, fb in (cases[m] if isinstance(cases, dict) else cases)]
    return pytest.mark.parametrize("mode,nch,fb", rows, ids=[_id(m, f"{'mono' if nch == 1 else 'stereo'}_{fb}") for m, nch, fb in rows])


_per_mode_and_channels = pytest.mark.parametrize("mode,nch", [(m, nch) for m in MODES for nch in (1, 2)],
                                                 ids=[_id(m, str(nch)) for m in MODES for nch in (1, 2)])


@pytest.fixture(scope="module")
def B():
    from atracdenc_amd import binding
    return binding


def _as16(pcm):
    p16 = np.clip(np.rint(pcm * 32767.0), -32768, 32767).astype(np.int16)
    return p16, (p16.astype(np.float32) / np.float32(32768.0)).astype(np.float32)


def _specs_of_pcm(pcm):
    """pcm [n, 2048, C] of one stream from its start -> [n, C, 2048]: what at3phip_encode_frames hands its writer"""
    out = np.zeros((pcm.shape[0], pcm.shape[2], 2048), np.float32)
    for c in range(pcm.shape[2]):
        bands = at3p_pqf(np.ascontiguousarray(pcm[:, :, c]))
        out[:, c] = at3p_mdct((bands.astype(np.float64) / G.SCALE).astype(np.float32))
    return out


_cache = {}


def _memo(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _plain(nch, frames=F):
    """(int16 PCM [n, frames, 2048, C], the same as float, the writer's spectra) of noise, tones and mix (2 streams for frames = 4)"""
    def make():
        names = ("noise", "tones", "mix") if frames == F else ("tones", "mix")
        p16, pcm = _as16(np.stack([G.signal_pcm(name, frames, nch) for name in names]))
        return p16, pcm, np.stack([_specs_of_pcm(pcm[s]) for s in range(len(names))])
    return _memo(("plain", nch, frames), make)


def _tonal(nch):
    """(int16 PCM, float PCM, residual spectra, the writer's records) of the tone analysis with gates and sharing"""
    def make():
        raw = [G.twin_pcm("tones", F), G.keyed_pcm(F, 2), G.twin_pcm("mix", F)] if nch == 2 else \
            [G.signal_pcm("tones", F, 1), G.keyed_pcm(F, 1), G.signal_pcm("mix", F, 1)]
        p16, pcm = _as16(np.stack(raw))
        specs, recs = [], []

        def grab(sp, rc):
            specs.append(sp)
            recs.append(rc)
            return np.zeros((sp.shape[0], 2048), np.uint8)
        for s in range(S):
            G.pipeline(pcm[s], True, True, grab)
        return p16, pcm, np.stack(specs), np.stack(recs)
    return _memo(("tonal", nch), make)


def _wspecs(nch):
    """the sparse tests' signals for the writer calls: noise, mix, tones"""
    return _memo(("wspecs", nch), lambda: np.stack([W.specs_of(n, nch, F) for n in ("noise", "mix", "tones")]))


def _corner_specs(mode, nch):
    """stream 0: an all-zero spectrum, a single non-zero line, a full-scale spectrum; stream 1: full-scale noise; stream 2: three of
    at3p_writer_lib.edge_specs' frames for rd, for psy two of them and then the masked twin (in the last channel)"""
    def make():
        sp = np.zeros((S, F, nch, 2048), np.float32)
        sp[0, 1, nch - 1, 777] = 0.3
        sp[0, 2] = np.where(np.random.default_rng(3).integers(0, 2, (nch, 2048)) > 0, 1.0, -1.0)
        sp[1] = W.full_scale_noise(F, nch)
        if mode == "rd":
            sp[2] = W.edge_specs(nch)[0][1:4]
        else:
            sp[2, :2] = W.edge_specs(nch)[0][1:3]
            sp[2, 2, nch - 1] = Y.masked_twin()[0, 0]
        return sp
    return _memo(("corner", mode, nch), make)


def _records(nch):
    small = TW.case_blocks(f"small_{nch}")[0][0]
    return [[TW.largest_block(nch), None, small], [None, TW.largest_block(nch), small], [None, small, None]]


def _want(mode, specs, fb, blocks=None):
    """the restatement's frames in the mode, [S, F, fb]; blocks [S][F] or None"""
    return np.stack([W.write_rd(specs[s], fb, None, None if blocks is None else blocks[s], psy=mode == "psy") for s in range(specs.shape[0])])


def _older(mode, specs, fb):
    """the restatement's frames in the mode's older mode: sparse for rd, rd for psy"""
    return W.write_streams(specs, fb, True) if mode == "rd" else _want("rd", specs, fb)


# ---- the writers -----------------------------------------------------------------------------------------------------------------
@_per_mode(CASES)
def test_six_calls_equal_the_restatement(B, mode, nch, fb):
    """host buffers: at3phip_write_frames, at3phip_write_frames_tonal, at3phip_encode_frames(_short), at3phip_encode_frames_tonal(_short)
    with gates and sharing; the corner spectra; and the frames are not the older mode's at the sizes where the budget binds"""
    KW = KWS[mode]
    p16, pcm, specs = _plain(nch)
    t16, tpcm, tspecs, trecs = _tonal(nch)
    wspecs, corner, blocks = _wspecs(nch), _corner_specs(mode, nch), _records(nch)
    recs = np.stack([B.pack_tonal_blocks(row, nch) for row in blocks])
    enc = B.At3pHip(n_streams=S, max_frames=F, channels=nch, frame_bytes=fb)
    try:
        got_w = enc.write_frames(wspecs, **KW)
        got_c = enc.write_frames(corner, **KW)
        got_t = enc.write_frames(wspecs, None, recs, **KW)
        got_ct = enc.write_frames(corner, None, recs, **KW)
        got_e = enc.encode_frames(pcm, **KW)
        enc.reset()
        got_e16 = enc.encode_frames_s16(p16, **KW)
        enc.reset()
        got_a = enc.encode_frames_tonal(tpcm, gated=True, shared=True, **KW)
        enc.reset()
        got_a16 = enc.encode_frames_tonal_s16(t16, gated=True, shared=True, **KW)
    finally:
        enc.close()
    want_w = _want(mode, wspecs, fb)
    assert np.array_equal(got_w, want_w)
    assert np.array_equal(got_c, _want(mode, corner, fb))
    assert np.array_equal(got_t, _want(mode, wspecs, fb, blocks))
    assert np.array_equal(got_ct, _want(mode, corner, fb, blocks))
    want_e = _want(mode, specs, fb)
    assert np.array_equal(got_e, want_e) and np.array_equal(got_e16, want_e)
    want_a = _want(mode, tspecs, fb, trecs)
    assert np.array_equal(got_a, want_a) and np.array_equal(got_a16, want_a)
    if fb < 2048:   # the flag matters where the budget binds
        older = _older(mode, wspecs, fb)
        if mode == "rd":
            assert not np.array_equal(want_w, older)
        else:       # no stream's frames are the rate-distortion writer's
            assert all(not np.array_equal(want_w[s], older[s]) for s in range(S))


@_per_mode(CASES)
def test_a_nan_and_an_infinity_in_one_stream_leave_the_others_alone(B, mode, nch, fb):
    """stream 1 holds a NaN and an infinity (and, a frame on, at3p_writer_lib.odd_specs' whole units of them): every stream equals the
    restatement, and streams 0 and 2 equal their encode beside a clean stream 1"""
    KW = KWS[mode]
    clean = _wspecs(nch)
    dirty = clean.copy()
    dirty[1, 0, 0, 100], dirty[1, 0, nch - 1, 1500] = np.nan, np.inf
    dirty[1, 1:] = W.odd_specs(nch, F - 1)
    enc = B.At3pHip(n_streams=S, max_frames=F, channels=nch, frame_bytes=fb)
    try:
        got, got_clean = enc.write_frames(dirty, **KW), enc.write_frames(clean, **KW)
    finally:
        enc.close()
    assert np.array_equal(got, _want(mode, dirty, fb))
    assert np.array_equal(got[0], got_clean[0]) and np.array_equal(got[2], got_clean[2]) and not np.array_equal(got[1], got_clean[1])


@_per_mode(DEVICE_CASES)
def test_device_buffers_queued_calls_splits_and_flag_switches(B, mode, nch, fb):
    """device buffers waiting and queued equal host buffers; one call of 3 frames equals calls of 1 + 2; a stream that switches the
    flag between calls gets each call's own frames; the bytes behind every output stay"""
    import torch
    p16, pcm, specs = _plain(nch)
    t16, tpcm, tspecs, trecs = _tonal(nch)
    KW = KWS[mode]
    want, want_older = _want(mode, specs, fb), _older(mode, specs, fb)
    t_want = _want(mode, tspecs, fb, trecs)
    n = S * F * fb
    DEV = B.AT3HIP_PCM_ON_DEVICE | B.AT3HIP_OUT_ON_DEVICE | B.AT3PHIP_ALLOC_ADAPTIVE | B.AT3PHIP_ALLOC_SPARSE | B.AT3PHIP_ALLOC_RD
    if mode == "psy":
        DEV |= B.AT3PHIP_ALLOC_PSY
    enc = B.At3pHip(n_streams=S, max_frames=F, channels=nch, frame_bytes=fb)
    try:
        d_pcm, d_specs, d_t16 = torch.from_numpy(pcm).cuda(), torch.from_numpy(specs).cuda(), torch.from_numpy(t16).cuda()
        outs = [torch.full((n + 4096,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(4)]
        torch.cuda.synchronize()
        enc.encode_frames_device(d_pcm.data_ptr(), F, outs[0].data_ptr(), **KW)
        enc.reset()
        enc.encode_frames_device(d_pcm.data_ptr(), F, outs[1].data_ptr(), asynchronous=True, **KW)
        enc.sync()
        enc.write_frames_ptr(d_specs.data_ptr(), F, None, outs[2].data_ptr(), DEV)
        enc.reset()
        enc.encode_frames_tonal_device_s16(d_t16.data_ptr(), F, outs[3].data_ptr(), asynchronous=True, gated=True, shared=True, **KW)
        enc.sync()

        def split(call, x, **k2):
            enc.reset()
            return np.concatenate([call(x[:, :1], **k2), call(x[:, 1:], **k2)], axis=1)
        parts = split(enc.encode_frames, pcm, **KW)
        t_parts = split(enc.encode_frames_tonal, tpcm, gated=True, shared=True, **KW)
        w_parts = np.concatenate([enc.write_frames(specs[:, :1], **KW), enc.write_frames(specs[:, 1:], **KW)], axis=1)
        enc.reset()
        switched = np.concatenate([enc.encode_frames(pcm[:, :1], **KW), enc.encode_frames(pcm[:, 1:2], **OLDER_KW[mode]),
                                   enc.encode_frames(pcm[:, 2:], **KW)], axis=1)
    finally:
        enc.close()
    got = [o.cpu().numpy() for o in outs]
    for g in got:
        assert (g[n:] == SENTINEL).all()
    for k in range(3):
        assert np.array_equal(got[k][:n].reshape(S, F, fb), want), k
    assert np.array_equal(got[3][:n].reshape(S, F, fb), t_want)
    assert np.array_equal(parts, want) and np.array_equal(w_parts, want) and np.array_equal(t_parts, t_want)
    assert np.array_equal(switched[:, 0], want[:, 0]) and np.array_equal(switched[:, 1], want_older[:, 1]) and np.array_equal(switched[:, 2], want[:, 2])


@_per_mode_and_channels
def test_pcm_in(B, mode, nch):
    """2 streams x 4 frames of PCM through at3phip_encode_frames and its 16-bit twin at 64 kbit/s per channel pair (376 bytes)"""
    KW = KWS[mode]
    p16, pcm, specs = _plain(nch, 4)
    enc = B.At3pHip(n_streams=2, max_frames=4, channels=nch, frame_bytes=376)
    try:
        got = enc.encode_frames(pcm, **KW)
        enc.reset()
        got16 = enc.encode_frames_s16(p16, **KW)
    finally:
        enc.close()
    want = _want(mode, specs, 376)
    assert np.array_equal(got, want) and np.array_equal(got16, want)


@_per_mode_and_channels
def test_the_flag_without_the_flags_it_needs_is_refused_and_moves_nothing(B, mode, nch):
    """AT3PHIP_ALLOC_RD alone, with ADAPTIVE only and with SPARSE only, AT3PHIP_ALLOC_PSY with any of ADAPTIVE, SPARSE and RD missing, on
    all six calls: AT3HIP_EINVAL with a last-error text, the output untouched, and the next valid call gives the bytes of a fresh stream
    (no filter-bank or analysis state moved)"""
    KW = KWS[mode]
    p16, pcm, specs = _plain(nch)
    recs = np.zeros((S, F), B.AT3P_TONAL_BLOCK_DTYPE)
    out = np.full((S, F, 2048), SENTINEL, np.uint8)
    enc = B.At3pHip(n_streams=S, max_frames=F, channels=nch)
    try:
        for names in LACKING[mode]:
            extra = sum(getattr(B, "AT3PHIP_ALLOC_" + n) for n in names)
            flag = getattr(B, FLAG[mode]) | extra
            calls = [lambda: enc.write_frames_ptr(specs.ctypes.data, F, None, out.ctypes.data, flag),
                     lambda: enc.write_frames_tonal_ptr(specs.ctypes.data, F, None, recs.ctypes.data, out.ctypes.data, flag),
                     lambda: enc.encode_frames_ptr(pcm.ctypes.data, F, out.ctypes.data, flag),
                     lambda: enc.encode_frames_s16_ptr(p16.ctypes.data, F, out.ctypes.data, flag),
                     lambda: enc.encode_frames_tonal_ptr(pcm.ctypes.data, F, out.ctypes.data, flag),
                     lambda: enc.encode_frames_tonal_s16_ptr(p16.ctypes.data, F, out.ctypes.data, flag)]
            for k, call in enumerate(calls):
                with pytest.raises(B.At3HipError, match=REFUSAL[mode]):
                    call()
                assert (out == SENTINEL).all(), (extra, k)
        for bad in BAD_KW[mode]:
            with pytest.raises(ValueError):
                enc.encode_frames(pcm, **bad)
        got = enc.encode_frames(pcm, **KW)
    finally:
        enc.close()
    assert np.array_equal(got, _want(mode, specs, 2048))


@_per_mode(DECODE_CASES)
def test_gpu_written_frames_decode_on_the_gpu_with_every_counter_zero(B, mode, nch, fb):
    """the writer's frames (records among them) through at3phip_decode with AT3PHIP_DECODE_TONES | AT3PHIP_DECODE_SPARSE: no frame
    rejected, and the PCM is the restatement decoder's"""
    KW = KWS[mode]
    wspecs, blocks = _wspecs(nch), _records(nch)
    recs = np.stack([B.pack_tonal_blocks(row, nch) for row in blocks])
    enc = B.At3pHip(n_streams=S, max_frames=F, channels=nch, frame_bytes=fb)
    dec = B.At3pHipDecoder(n_streams=S, channels=nch, max_frames=F, frame_bytes=fb)
    try:
        frames = enc.write_frames(wspecs, None, recs, **KW)
        pcm = dec.decode(frames, tones=True, sparse=True)
        cnt = dec.counters()
    finally:
        enc.close()
        dec.close()
    want, rej = W.decode_streams(frames, nch, True, True)
    assert sum(cnt.values()) == 0 == rej.sum(), (cnt, rej)
    assert np.array_equal(pcm.view(np.uint32), want.view(np.uint32))
