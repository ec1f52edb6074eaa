"""at3hipenc's text: the banners on stdout, the messages on stderr and the exit status of every encoder and decoder, compared
whole with what the tool printed before its decode and encode paths were folded into one driver each (EXPECTED below, file
paths reduced to their names; recorded from that earlier tool, linked against the library built through tools/emu). One
16 384-sample input: 32 ATRAC1 blocks, 16 ATRAC3 blocks, 8 ATRAC3plus frames."""
import os
import subprocess

import numpy as np
import pytest

from test_resample_cli_gpu import CLI, write_wav

pytestmark = pytest.mark.gpu

N = 16384


def _corrupt_at3(d):
    """frame 3 of the OMA starts with a byte whose upper six bits are not the unit id 0x28"""
    data = bytearray(open(d / "st3.oma", "rb").read())
    data[96 + 3 * 384] = 0x00
    open(d / "bad3.oma", "wb").write(bytes(data))


def _corrupt_at3p(d):
    """frame 2 of the OMA is a crafted frame whose first bit is set: counted under 'bad header or block type'"""
    from at3p_decode_lib import _small_mant, make_frame
    nq = 6
    bad = make_frame(2, first_bit=1, nqu=nq, wl=[[3] * nq] * 2, sf=[[30 + q for q in range(nq)]] * 2, mant=_small_mant)
    data = bytearray(open(d / "stp.oma", "rb").read())
    data[96 + 2 * 2048:96 + 3 * 2048] = bad.tobytes()
    open(d / "badp.oma", "wb").write(bytes(data))


# name: (what must have run before, the tool's arguments; a name with a dot is a file in the test's directory)
CASES = {
    "enc_atrac1": ((), "-e atrac1 -i st.wav -o st.aea"),
    "enc_atrac3": ((), "-e atrac3 -i st.wav -o st3.oma"),
    "enc_atrac3plus": ((), "-e atrac3plus -i st.wav -o stp.oma"),
    "enc_atrac1_mono": ((), "-e atrac1 -i mono.wav -o mono.aea"),
    "enc_atrac3plus_mono": ((), "-e atrac3plus -i mono.wav -o monop.oma"),
    "dec_atrac1": (("enc_atrac1",), "-d -i st.aea -o st1.wav"),
    "dec_atrac3": (("enc_atrac3",), "-d -i st3.oma -o st3.wav"),
    "dec_atrac3plus": (("enc_atrac3plus",), "-d -i stp.oma -o stp.wav"),
    "dec_atrac1_mono": (("enc_atrac1_mono",), "-d -i mono.aea -o mono1.wav"),
    "dec_atrac3plus_mono": (("enc_atrac3plus_mono",), "-d -i monop.oma -o monop.wav"),
    "dec_atrac3_rate": (("enc_atrac3",), "-d -i st3.oma -o st3_48k.wav --rate 48000"),
    "dec_atrac1_batch3": (("enc_atrac1",), "-d -i st.aea -o st1_b3.wav --batch 3"),
    "dec_atrac3_batch3": (("enc_atrac3",), "-d -i st3.oma -o st3_b3.wav --batch 3"),
    "dec_atrac3plus_batch3": (("enc_atrac3plus",), "-d -i stp.oma -o stp_b3.wav --batch 3"),
    "dec_atrac3_wrong_unit_id": (("enc_atrac3", _corrupt_at3), "-d -i bad3.oma -o bad3.wav"),
    "dec_atrac3plus_bad_header": (("enc_atrac3plus", _corrupt_at3p), "-d -i badp.oma -o badp.wav"),
}

# (exit status, stdout, stderr): what the tool printed for these inputs before the drivers were shared
EXPECTED = {
    "enc_atrac1": (0,
        "Input\n Filename: st.wav\n Channels: 2\n SampleRate: 44100\n Duration (sec): 0\nOutput:\n Filename: st.aea\n Codec: ATRAC1\n\nDone\n",
        ""),
    "enc_atrac3": (0,
        "Input:\n Filename: st.wav\n Channels: 2\n SampleRate: 44100\n Duration (sec): 0\nOutput:\n Filename: st3.oma\n Codec: ATRAC3\n Bitrate: 132300\n\nDone\n",
        ""),
    "enc_atrac3plus": (0,
        "Input:\n Filename: st.wav\n Channels: 2\n SampleRate: 44100\n Duration (sec): 0\nOutput:\n Filename: stp.oma\n Codec: ATRAC3Plus\n\nDone\n",
        ""),
    "enc_atrac1_mono": (0,
        "Input\n Filename: mono.wav\n Channels: 1\n SampleRate: 44100\n Duration (sec): 0\nOutput:\n Filename: mono.aea\n Codec: ATRAC1\n\nDone\n",
        ""),
    "enc_atrac3plus_mono": (0,
        "Input:\n Filename: mono.wav\n Channels: 1\n SampleRate: 44100\n Duration (sec): 0\nOutput:\n Filename: monop.oma\n Codec: ATRAC3Plus\n\nDone\n",
        ""),
    "dec_atrac1": (0,
        "Input\n Filename: st.aea\n Name: test\n Channels: 2\nOutput:\n Filename: st1.wav\n Codec: PCM\n\nDone\n",
        ""),
    "dec_atrac3": (0,
        "Input\n Filename: st3.oma\n Container: OMA\n Codec: ATRAC3, frame size 384\nOutput:\n Filename: st3.wav\n Codec: PCM\n\nDone\n",
        ""),
    "dec_atrac3plus": (0,
        "Input\n Filename: stp.oma\n Container: OMA\n Codec: ATRAC3plus, 2 channels\nOutput:\n Filename: stp.wav\n Codec: PCM\n\nDone\n",
        ""),
    "dec_atrac1_mono": (0,
        "Input\n Filename: mono.aea\n Name: test\n Channels: 1\nOutput:\n Filename: mono1.wav\n Codec: PCM\n\nDone\n",
        ""),
    "dec_atrac3plus_mono": (0,
        "Input\n Filename: monop.oma\n Container: OMA\n Codec: ATRAC3plus, 1 channel\nOutput:\n Filename: monop.wav\n Codec: PCM\n\nDone\n",
        ""),
    "dec_atrac3_rate": (0,
        "Input\n Filename: st3.oma\n Container: OMA\n Codec: ATRAC3, frame size 384\nOutput:\n Filename: st3_48k.wav\n Codec: PCM\n\nDone\n",
        ""),
    "dec_atrac1_batch3": (0,
        "Input\n Filename: st.aea\n Name: test\n Channels: 2\nOutput:\n Filename: st1_b3.wav\n Codec: PCM\n\nDone\n",
        ""),
    "dec_atrac3_batch3": (0,
        "Input\n Filename: st3.oma\n Container: OMA\n Codec: ATRAC3, frame size 384\nOutput:\n Filename: st3_b3.wav\n Codec: PCM\n\nDone\n",
        ""),
    "dec_atrac3plus_batch3": (0,
        "Input\n Filename: stp.oma\n Container: OMA\n Codec: ATRAC3plus, 2 channels\nOutput:\n Filename: stp_b3.wav\n Codec: PCM\n\nDone\n",
        ""),
    "dec_atrac3_wrong_unit_id": (0,
        "Input\n Filename: bad3.oma\n Container: OMA\n Codec: ATRAC3, frame size 384\nOutput:\n Filename: bad3.wav\n Codec: PCM\n\nDone\n",
        "Skipped invalid ATRAC3 units (wrong unit id): 1\n"),
    "dec_atrac3plus_bad_header": (0,
        "Input\n Filename: badp.oma\n Container: OMA\n Codec: ATRAC3plus, 2 channels\nOutput:\n Filename: badp.wav\n Codec: PCM\n\nDone\n",
        "Skipped invalid ATRAC3plus frames (bad header or block type): 1\n"),
}


class Session:
    """runs each case once, after what it needs, in one directory"""

    def __init__(self, d):
        self.d = d
        self.done = {}
        rng = np.random.RandomState(5)
        t = np.arange(N)
        x = np.stack([0.5 * np.sin(2 * np.pi * 997 * t / 44100) + 0.1 * rng.uniform(-1, 1, N),
                      0.4 * np.sin(2 * np.pi * 5000 * t / 44100 + 1) + 0.05 * rng.uniform(-1, 1, N)], axis=-1)
        s16 = np.clip(np.round(x * 32767), -32768, 32767).astype(np.int16)
        write_wav(str(d / "st.wav"), s16, 44100)
        write_wav(str(d / "mono.wav"), s16[:, :1], 44100)

    def get(self, name):
        if name not in self.done:
            needs, args = CASES[name]
            for need in needs:
                if callable(need):
                    need(self.d)
                else:
                    assert self.get(need)[0] == 0, (need, self.done[need])
            argv = [str(self.d / a) if "." in a else a for a in args.split()]
            r = subprocess.run([CLI, *argv], capture_output=True, text=True, timeout=120)
            prefix = str(self.d) + os.sep
            self.done[name] = (r.returncode, r.stdout.replace(prefix, ""), r.stderr.replace(prefix, ""))
        return self.done[name]


@pytest.fixture(scope="module")
def session(tmp_path_factory):
    return Session(tmp_path_factory.mktemp("cli_text"))


@pytest.mark.parametrize("name", list(CASES))
def test_cli_text(session, name):
    got = session.get(name)
    print(repr(got))
    assert got == EXPECTED[name]
