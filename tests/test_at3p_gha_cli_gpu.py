"""at3hipenc -e atrac3plus --tones: the file decodes (no frame is skipped, the PCM is the decoder's for these frames), differs from the plain file on `tones`, holds the plain
file's frame count, and its frames are at3phip_encode_frames_tonal's; without the flag the file is the plain schedule's, frame for
frame: the silent frame, then at3phip_encode_frames' frames."""
import os
import subprocess
import wave

import numpy as np
import pytest

import at3p_gha_lib as G

pytestmark = pytest.mark.gpu
NF = 8


def _frames(path):
    data = open(path, "rb").read()
    assert data[:3] == b"EA3"
    body = data[96:]
    return np.frombuffer(body[:len(body) // 2048 * 2048], np.uint8).reshape(-1, 2048)


@pytest.mark.parametrize("nch", [1, 2])
def test_cli_tones(tmp_path, nch):
    from atracdenc_amd import binding as B
    exe = os.path.join(os.path.dirname(B.LIB_PATH), "at3hipenc")
    pcm16 = np.clip(np.rint(G.signal_pcm("tones", NF, nch) * 32767.0), -32768, 32767).astype("<i2")
    wav_in = str(tmp_path / "in.wav")
    with wave.open(wav_in, "wb") as w:
        w.setnchannels(nch)
        w.setsampwidth(2)
        w.setframerate(44100)
        w.writeframes(pcm16.tobytes())
    plain, tonal, wav_out = str(tmp_path / "plain.oma"), str(tmp_path / "tonal.oma"), str(tmp_path / "y.wav")
    for out, extra in ((plain, []), (tonal, ["--tones", "--batch", "3"])):
        r = subprocess.run([exe, "-e", "atrac3plus", "-i", wav_in, "-o", out, "--nostdout", *extra], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
    fp, ft = _frames(plain), _frames(tonal)
    # (the reader's schedule owes the look-ahead call one more: NF + 1 calls, NF frames; that call is the flushing frame)
    assert fp.shape == ft.shape == (NF, 2048)
    assert open(plain, "rb").read()[:96] == open(tonal, "rb").read()[:96]       # the same header: the same frame count
    assert (fp != ft).any(axis=1).sum() >= NF - 1                                # tones are found from the first pair on
    # the input as the tool's reader hands it to the encoder: int16 / 32768
    x = (pcm16.astype(np.float32) / np.float32(32768.0)).reshape(1, NF, 2048, nch)
    enc = B.At3pHip(n_streams=1, max_frames=NF, channels=nch)
    try:
        want_tonal = enc.encode_frames_tonal(x)[0]
        enc.reset()
        want_plain = enc.encode_frames(x)[0]
        silent = enc.write_frames(np.zeros((1, 1, nch, 2048), np.float32))[0, 0]
    finally:
        enc.close()
    assert np.array_equal(ft, want_tonal)   # (frame f needs the input up to frame f only)
    assert np.array_equal(fp[0], silent) and np.array_equal(fp[1:], want_plain[:NF - 1])   # without the flag: the schedule as it was
    r = subprocess.run([exe, "-d", "-i", tonal, "-o", wav_out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Skipped" not in r.stdout + r.stderr, r.stdout + r.stderr
    dec = B.At3pHipDecoder(n_streams=1, channels=nch, max_frames=NF)
    try:
        want = dec.decode(ft[None], s16=True, tones=True)[0].reshape(-1, nch)
        assert sum(dec.counters().values()) == 0
    finally:
        dec.close()
    with wave.open(wav_out, "rb") as w:
        got = np.frombuffer(w.readframes(w.getnframes()), "<i2").reshape(-1, nch)
    assert np.array_equal(got, want)
