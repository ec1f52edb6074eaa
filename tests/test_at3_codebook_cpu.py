"""Every ATRAC3 mantissa code at every bit phase, without a GPU (at3_decode_lib.code_corpus): the C restatement's unpack against
the spectrum computed in numpy from the symbols the corpus was written from, and the seven selectors' prefix-code properties."""
from fractions import Fraction

import numpy as np
import pytest

import at3_decode_lib as A


def test_tables_are_complete_prefix_codes():
    tables = A.vlc_tables()
    assert sum(len(tables[s]) for s in (1, 2, 3, 5, 6, 7)) == 130 and tables[4] == tables[1]
    assert tables[1] == A.HUFF[1] and tables[2] == A.HUFF[2] and tables[3] == A.HUFF[3]
    for s, t in tables.items():
        assert sum(Fraction(1, 1 << n) for _, n in t) == 1, s
        words = sorted(format(code, f"0{n}b") for code, n in t)
        assert not any(b.startswith(a) for a, b in zip(words, words[1:])), s
        assert max(n for _, n in t) <= 8


@pytest.mark.parametrize("js", [False, True], ids=["plain", "joint-stereo"])
def test_unpack_equals_numpy_expectation(js):
    """(float32(m) * ScaleTable[sf]) * InvMaxQuant[wl] of the intended mantissas, as bit patterns; no unit rejected, every unit VLC"""
    c = A.code_corpus(js)
    assert c["frame_sz"] == (192 if js else 304)
    frames = c["frames"].reshape(-1, c["frame_sz"])
    spec, fl = A.unpack(frames, c["frame_sz"], js)
    assert not fl["reason"].any() and not fl["coding_mode"].any()
    assert np.array_equal(fl["wl"], c["wl"].reshape(-1, 2, 32)) and np.array_equal(fl["n_points"][:, :, 0], np.repeat(np.arange(32) % 4, 7)[:, None] + [0, 0])
    want = A.corpus_expected_spectrum(c).reshape(-1, 2, 1024)
    assert np.array_equal(spec.view(np.uint32), want.view(np.uint32))
