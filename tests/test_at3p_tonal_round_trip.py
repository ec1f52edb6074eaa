"""The tonal block's alignment (include/at3phip.h, step 4b): tones subtracted from the subband signal as the reference encoder's
ApplyFilter does, the residual encoded, each block written one frame late as TAt3PEnc writes `delay`, then decoded. The
reconstruction must come close to the round trip without tones, and shifting the blocks by one frame either way must cost at
least 10 dB."""
import numpy as np

import at3p_tonal_lib as L
from at3_testlib import _vp, at3p_mdct, at3p_pqf, at3p_signal, at3p_write_frames
from at3p_decode_lib import DELAY

NF = 14
# measured on this test: 15.63 dB with the tones against 15.90 dB without them; blocks shifted by -1 / +1 frame give 3.77 / 4.25 dB
FLOOR_DB = 1.0


def _block(j):
    """large hand-chosen tones in two bands, one fading in and one out, none in frame 5"""
    if j == 5:
        return None
    return {"nb": 3, "shared": [False] * 3, "leader": False,
            "bands": [[{"start": None, "stop": None, "waves": [(90, 50, 3), (400, 46, 17)]},
                       {"start": None, "stop": None, "waves": []},
                       {"start": 4 if j == 7 else None, "stop": 20 if j == 10 else None, "waves": [(700, 48, 9)]}]]}


def _records():
    return [L.unpack_tonal(L.make_tonal_frame(1, b)[None], 1)[2][0] if b else np.zeros(L.REC_INTS, np.int32)
            for b in map(_block, range(NF))]


def _encode(bands):
    b = (bands.astype(np.float64) / (32768.0 / 1.122018)).astype(np.float32)
    return at3p_write_frames(at3p_mdct(b.reshape(-1, 16, 128))[:, None, :])


def _snr(x, y):
    n = x.shape[0] - DELAY
    ref, out = x[:n], y[DELAY:DELAY + n]
    return 10 * np.log10(np.sum(ref.astype(np.float64) ** 2) / np.sum((ref - out).astype(np.float64) ** 2))


def test_tonal_blocks_go_with_their_own_frame():
    x2 = at3p_signal("mix", NF, channel=0, scale=0.5)
    x = x2.reshape(-1)
    bands = at3p_pqf(x2).reshape(NF, 2048)
    # the encoder: ApplyFilter(T_j) on frame j's subband samples, the residual through the MDCT and the writer
    lib = L.tonal_lib()
    st = np.zeros(lib.at3pt_filter_bytes(), np.uint8)
    resid = bands.astype(np.float32).copy()
    for j, r in enumerate(_records()):
        lib.at3pt_apply_filter(_vp(st), 1, _vp(np.ascontiguousarray(r)), _vp(resid[j]))
    assert np.abs(resid - bands).max() > 1000.0   # the tones are large against the signal
    base = _encode(resid)
    plain = _encode(bands.astype(np.float32))

    def frames(shift):
        # frame j carries the block of frame j - 1 (TAt3PEnc writes `delay`); shift moves it
        out = []
        for j in range(NF):
            k = j - 1 + shift
            b = _block(k) if 0 <= k < NF else None
            out.append(base[j] if b is None else L.splice_tonal(base[j], L.tonal_bits(1, b)))
        return np.stack(out)

    snr = {}
    for shift in (-1, 0, 1):
        pcm, rej = L.cpu_tonal_decode(frames(shift), 1)
        assert rej.sum() == 0
        snr[shift] = _snr(x, pcm[:, :, 0].reshape(-1))
    pcm, _ = L.cpu_tonal_decode(plain, 1)
    snr_plain = _snr(x, pcm[:, :, 0].reshape(-1))
    assert snr[0] >= snr_plain - FLOOR_DB, (snr, snr_plain)
    assert snr[0] >= snr[-1] + 10.0 and snr[0] >= snr[1] + 10.0, snr
