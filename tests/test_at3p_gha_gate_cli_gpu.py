"""at3hipenc -e atrac3plus --tones --gate: the file holds the plain file's frame count and its frames are those of the gated
analysis - at3phip_encode_frames_tonal with AT3PHIP_TONES_GATED, which are the frames the host mirror writes with
TAt3PToneAnalyser(channels, gated) (tests/test_at3p_gha_gate_cpu.py pins the mirror to the same restatement pipeline this test
compares with); it differs from the --tones file where the signal has an onset, and decodes without a skipped frame. --gate without
--tones is a usage error."""
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
def test_cli_tones_gate(tmp_path, nch):
    from atracdenc_amd import binding as B
    exe = os.path.join(os.path.dirname(B.LIB_PATH), "at3hipenc")
    pcm16 = np.clip(np.rint(G.keyed_pcm(NF, nch) * 32767.0), -32768, 32767).astype("<i2")
    wav_in = str(tmp_path / "in.wav")
    with wave.open(wav_in, "wb") as w:
        w.setnchannels(nch)
        w.setsampwidth(2)
        w.setframerate(44100)
        w.writeframes(pcm16.tobytes())
    plain, tonal, gated, wav_out = str(tmp_path / "plain.oma"), str(tmp_path / "tonal.oma"), str(tmp_path / "gated.oma"), str(tmp_path / "y.wav")
    for out, extra in ((plain, []), (tonal, ["--tones", "--batch", "3"]), (gated, ["--tones", "--gate", "--batch", "3"])):
        r = subprocess.run([exe, "-e", "atrac3plus", "-i", wav_in, "-o", out, "--nostdout", *extra], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
    fp, ft, fg = _frames(plain), _frames(tonal), _frames(gated)
    assert fp.shape == ft.shape == fg.shape == (NF, 2048)
    assert open(plain, "rb").read()[:96] == open(gated, "rb").read()[:96]       # the same header: the plain frame count
    assert (fg != ft).any()                                                      # keyed has onsets and offsets
    # the input as the tool's reader hands it to the encoder: int16 / 32768
    x = (pcm16.astype(np.float32) / np.float32(32768.0)).reshape(NF, 2048, nch)
    enc = B.At3pHip(n_streams=1, max_frames=NF, channels=nch)
    try:
        want = G.pipeline(x, True, False, lambda specs, recs: enc.write_frames(specs[None], None, recs[None])[0])[0]
        enc.reset()
        want_gpu = enc.encode_frames_tonal(x[None], gated=True)[0]
    finally:
        enc.close()
    assert np.array_equal(fg, want) and np.array_equal(fg, want_gpu)
    r = subprocess.run([exe, "-d", "-i", gated, "-o", wav_out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Skipped" not in r.stdout + r.stderr, r.stdout + r.stderr
    r = subprocess.run([exe, "-e", "atrac3plus", "-i", wav_in, "-o", str(tmp_path / "bad.oma"), "--nostdout", "--gate"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
