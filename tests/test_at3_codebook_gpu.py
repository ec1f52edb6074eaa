"""Every ATRAC3 mantissa code at every bit phase on the GPU (at3_decode_lib.code_corpus: 32 streams, one per shift, of one frame per
selector), in plain units and in the byte-reversed second unit of joint-stereo frames: the decoder's PCM is the C restatement's bit
for bit and no unit is rejected. Every frame is valid."""
import numpy as np
import pytest

import at3_decode_lib as A

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("js", [False, True], ids=["plain", "joint-stereo"])
def test_corpus_equals_restatement(js):
    from atracdenc_amd import At3HipDecoder
    c = A.code_corpus(js)
    frames = c["frames"]
    dec = At3HipDecoder(n_streams=frames.shape[0], frame_size=c["frame_sz"], max_frames=frames.shape[1])
    assert dec.joint_stereo == js
    got = dec.decode(frames)
    counters = dec.counters()
    dec.close()
    want, rejected = A.cpu_ref(frames, c["frame_sz"], js)
    assert not any(rejected) and all(counters[r] == 0 for r in A.REASONS), (rejected, counters)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
