"""at3hipenc -e atrac3plus --adaptive --sparse --rd and, in the second mode, --psy beside them: at 64 kbit/s the file's frames are the
binding's (at3phip_encode_frames with ADAPTIVE | SPARSE | RD (| PSY) behind the host's one-frame lead-in) and differ from the file
written without the mode's option; -d decodes it with no frame skipped, to the decoder's PCM for these frames; --rd without --sparse,
--psy without --rd exits with its message and writes no file."""
import os
import subprocess
import wave

import numpy as np
import pytest

import at3p_gha_lib as G
import at3p_writer_lib as W

pytestmark = pytest.mark.gpu
NF, FB = 9, 376
# per mode: the command line's options, those of the older mode the file must differ from, the option sets that are refused and the message
OPTIONS = {"rd": ["--adaptive", "--sparse", "--rd"], "psy": ["--adaptive", "--sparse", "--rd", "--psy"]}
OLDER = {"rd": ["--adaptive", "--sparse"], "psy": ["--adaptive", "--sparse", "--rd"]}
REFUSED = {"rd": (["--adaptive", "--rd"], ["--rd"]), "psy": (["--adaptive", "--sparse", "--psy"], ["--psy"])}
MESSAGE = {"rd": "--rd needs --adaptive --sparse", "psy": "--psy needs --adaptive --sparse --rd"}


def _run(*args):
    return subprocess.run(list(args), capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("mode", ["rd", "psy"])
def test_cli(tmp_path, mode, nch):
    from atracdenc_amd import binding as B
    exe = os.path.join(os.path.dirname(B.LIB_PATH), "at3hipenc")
    pcm16 = np.clip(np.rint(G.signal_pcm("mix", NF, nch) * 32767.0), -32768, 32767).astype("<i2")
    wav_in, oma, plain, wav_out = str(tmp_path / "in.wav"), str(tmp_path / "mode.oma"), str(tmp_path / "older.oma"), str(tmp_path / "y.wav")
    with wave.open(wav_in, "wb") as w:
        w.setnchannels(nch)
        w.setsampwidth(2)
        w.setframerate(44100)
        w.writeframes(pcm16.tobytes())
    for args in REFUSED[mode]:
        r = _run(exe, "-e", "atrac3plus", "-i", wav_in, "-o", oma, *args, "--bitrate", "352")
        assert r.returncode != 0 and MESSAGE[mode] in r.stderr and not os.path.exists(oma), r.stdout + r.stderr
    r = _run(exe, "-e", "atrac3plus", "-i", wav_in, "-o", oma, *OPTIONS[mode], "--bitrate", "64", "--batch", "4")
    assert r.returncode == 0 and "Bitrate: 64 kbit/s (376-byte frames)" in r.stdout, r.stdout + r.stderr
    r = _run(exe, "-e", "atrac3plus", "-i", wav_in, "-o", plain, *OLDER[mode], "--bitrate", "64", "--nostdout")
    assert r.returncode == 0, r.stderr
    data = open(oma, "rb").read()
    assert len(data) == 96 + NF * FB and data[96:] != open(plain, "rb").read()[96:]
    got = np.frombuffer(data[96:], np.uint8).reshape(NF, FB)
    x = (pcm16.astype(np.float32) / np.float32(32768.0)).reshape(1, NF, 2048, nch)
    enc = B.At3pHip(n_streams=1, max_frames=NF, channels=nch, frame_bytes=FB)
    dec = B.At3pHipDecoder(n_streams=1, channels=nch, max_frames=NF, frame_bytes=FB)
    try:
        lib_frames = enc.encode_frames(x, adaptive=True, sparse=True, rd=True, psy=mode == "psy")[0]
        want = np.concatenate([W.write_rd(np.zeros((1, nch, 2048), np.float32), FB, psy=mode == "psy"), lib_frames[:NF - 1]])   # the host's one-frame lead-in
        assert np.array_equal(got, want)
        lib_pcm = dec.decode(want[None], s16=True, tones=True, sparse=True)[0]
        assert sum(dec.counters().values()) == 0
    finally:
        enc.close()
        dec.close()
    r = _run(exe, "-d", "-i", oma, "-o", wav_out)
    assert r.returncode == 0 and "Skipped" not in r.stdout + r.stderr, r.stdout + r.stderr
    with wave.open(wav_out, "rb") as w:
        assert np.array_equal(np.frombuffer(w.readframes(NF * 2048), "<i2").reshape(NF, 2048, nch), lib_pcm)
