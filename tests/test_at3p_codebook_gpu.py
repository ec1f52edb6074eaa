"""Every ATRAC3plus spectrum code at every bit phase on the GPU (at3p_decode_lib.code_corpus: 32 streams, one per shift, of one frame
per table, the group-flag frames and the frame that ends on its limit): the decoder's PCM is the C restatement's bit for bit and no
frame is rejected. Every frame is valid; corrupt input is test_fuzz_equals_restatement's business. And the fixed writer on spectra that
steer it through the tables (at3p_decode_lib.steered_spectra): its frames are the C restatement's byte for byte."""
import numpy as np
import pytest

import at3p_decode_lib as D
import at3p_writer_lib as W

pytestmark = pytest.mark.gpu

# channels, sparse, sized (the corpus' smallest standard frame size; otherwise 2048 and the setter is not called)
SHAPES = [(1, False, False), (1, True, True), (2, False, True), (2, True, False)]


@pytest.mark.parametrize("nch,sparse,sized", SHAPES, ids=["mono-plain-2048", "mono-sparse-sized", "stereo-plain-sized", "stereo-sparse-2048"])
def test_corpus_equals_restatement(nch, sparse, sized):
    import atracdenc_amd
    c = D.code_corpus(nch)
    fb = c["bytes"] if sized else D.FRAME
    frames = np.ascontiguousarray(c["frames"][:, :, :fb])
    S, F = frames.shape[:2]
    dec = atracdenc_amd.At3pHipDecoder(n_streams=S, channels=nch, max_frames=F, device_id=0, frame_bytes=fb if sized else None)
    got = dec.decode(frames, sparse=sparse)
    counters = dec.counters()
    dec.close()
    want, rejected = W.decode_streams(frames, nch, sparse=sparse)
    assert not rejected.any(), rejected
    assert all(counters[r] == 0 for r in D.REASONS), counters
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.argwhere((got.view(np.uint32) != want.view(np.uint32)).any(axis=(2, 3)))[:8]


@pytest.mark.parametrize("nch", [1, 2], ids=["mono", "stereo"])
def test_steered_writer_equals_restatement(oracle, nch):
    """the writer's code look-up and the two-word split of its bit writer, on codes the test signals never emit"""
    import atracdenc_amd
    from at3_testlib import at3p_write_frames
    specs, _, _ = D.steered_spectra(nch)
    S, F = specs.shape[:2]
    enc = atracdenc_amd.At3pHip(n_streams=S, max_frames=F, channels=nch, device_id=0)
    got = enc.write_frames(specs)
    enc.close()
    want = at3p_write_frames(specs.reshape(S * F, nch, D.FRAME)).reshape(S, F, D.FRAME)
    assert np.array_equal(got, want), np.argwhere((got != want).any(axis=2))[:8]
