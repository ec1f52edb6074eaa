"""at3phip_write_frames_tonal on the GPU: the reference's frames bit for bit (tests/golden/at3p_tonal_write.npz: spectra from the
stored seeds, blocks from the stored ints, 2 streams x 3 frames with a frame without a block between two with one), its
equivalences with at3phip_write_frames, its buffer and queueing flags, and the written blocks through the decoder."""
import numpy as np
import pytest

import at3p_tonal_lib as T
import at3p_tonal_write_lib as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return np.load(L.GOLDEN)


@pytest.fixture(scope="module")
def B():
    from atracdenc_amd import binding
    return binding


def _case(golden, B, cid):
    nch = int(cid.rsplit("_", 1)[1])
    blocks = L.blocks_from_ints(nch, golden[f"{cid}_blocks"])
    flags = golden[f"{cid}_flags"] if f"{cid}_flags" in golden else None
    return nch, L.case_specs(cid, int(golden[f"{cid}_seed"])), flags, blocks, B.pack_tonal_blocks(blocks, nch)


def _write(B, nch, specs, flags, recs):
    enc = B.At3pHip(n_streams=specs.shape[0], max_frames=specs.shape[1], channels=nch)
    try:
        return enc.write_frames(specs, flags, recs)
    finally:
        enc.close()


# what each case holds (tests/at3p_tonal_write_lib.py): small - one band with one wave, an envelope without waves, 15 waves in a band,
# 16 bands with 48 waves and both envelope points; freq - frequency lists that make ascending cheaper, descending cheaper and equal
# (takes descending), predecessors of 512 and above, equal frequencies; steep - windows in the `1 1` form (and `1 0`, and sine) next
# to blocks; share_a / share_b - sharing none, some and all, each with and without the leader flag; random - blocks drawn at random;
# loud - loud white spectra, the largest block
@pytest.mark.parametrize("cid", L.writer_case_ids())
def test_frames_equal_the_reference(golden, B, cid):
    nch, specs, flags, blocks, recs = _case(golden, B, cid)
    assert recs.shape == (L.STREAMS, L.FRAMES)
    for row in blocks:   # a frame without a block sits between two with one
        assert row[0] is not None and row[1] is None and row[2] is not None
    got = _write(B, nch, specs, flags, recs)
    bad = (got != golden[f"{cid}_frames"]).any(axis=2)
    assert not bad.any(), np.argwhere(bad).tolist()


def test_the_block_lowers_the_unit_count(golden, B):
    """Loud stereo white spectra: with the largest block fewer quant units are kept than for the same spectra without a block
    (the tail's bits count in CheckFrameDone); the frames are the reference's, which shows the same difference."""
    nch, specs, flags, blocks, recs = _case(golden, B, "loud_2")
    with_block = _write(B, nch, specs, flags, recs)
    without = _write(B, nch, specs, flags, None)
    assert np.array_equal(with_block, golden["loud_2_frames"])
    seen = 0
    for s in range(L.STREAMS):
        for f in range(L.FRAMES):
            if blocks[s][f] is None:
                assert np.array_equal(with_block[s, f], without[s, f])
            elif blocks[s][f]["nb"] == 16:
                assert T.n_qu(with_block[s, f]) < T.n_qu(without[s, f]), (s, f)
                seen += 1
            assert T.n_qu(with_block[s, f]) <= T.n_qu(without[s, f])
    assert seen >= 2


@pytest.mark.parametrize("nch", [1, 2])
def test_no_records_and_zero_records_equal_write_frames(golden, B, nch):
    """tonal = NULL and all-zero records are at3phip_write_frames, with and without window flags."""
    cid = f"steep_{nch}"
    _, specs, flags, _, recs = _case(golden, B, cid)
    enc = B.At3pHip(n_streams=L.STREAMS, max_frames=L.FRAMES, channels=nch)
    try:
        for fl in (None, flags):
            want = enc.write_frames(specs, fl)
            out = np.zeros_like(want)
            enc.write_frames_tonal_ptr(specs.ctypes.data, L.FRAMES, None if fl is None else fl.ctypes.data, None, out.ctypes.data, 0)
            assert np.array_equal(out, want)
            assert np.array_equal(enc.write_frames(specs, fl, np.zeros_like(recs)), want)
            # zero records next to a block go through the instantiation with records: still the writer without records
            mixed = np.zeros_like(recs)
            mixed[0, 0] = recs[0, 0]
            got = enc.write_frames(specs, fl, mixed)
            assert np.array_equal(got.reshape(-1, 2048)[1:], want.reshape(-1, 2048)[1:]) and not np.array_equal(got[0, 0], want[0, 0])
    finally:
        enc.close()


def test_device_buffers_and_a_queued_call_in_front(golden, B):
    """Host and device specs / frames in all four combinations give the same frames, and so does a call (with AT3HIP_ASYNC in its
    flags, which the stage-level calls accept and wait regardless) behind a queued at3phip_encode_frames whose writer is still
    running on the context's second stream."""
    import torch
    nch, specs, flags, _, recs = _case(golden, B, "random_2")
    want = golden["random_2_frames"]
    enc = B.At3pHip(n_streams=L.STREAMS, max_frames=L.FRAMES, channels=nch)
    try:
        d_specs = torch.from_numpy(specs).cuda()
        torch.cuda.synchronize()
        for in_dev in (False, True):
            for out_dev in (False, True):
                h_out = np.zeros((L.STREAMS, L.FRAMES, 2048), np.uint8)
                d_out = torch.zeros((L.STREAMS, L.FRAMES, 2048), dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                enc.write_frames_tonal_ptr(d_specs.data_ptr() if in_dev else specs.ctypes.data, L.FRAMES, None, recs.ctypes.data,
                                           d_out.data_ptr() if out_dev else h_out.ctypes.data,
                                           (B.AT3HIP_PCM_ON_DEVICE if in_dev else 0) | (B.AT3HIP_OUT_ON_DEVICE if out_dev else 0))
                got = d_out.cpu().numpy() if out_dev else h_out
                assert np.array_equal(got, want), (in_dev, out_dev)
        pcm = torch.from_numpy((0.1 * np.random.RandomState(9).standard_normal((L.STREAMS, L.FRAMES, 2048, nch))).astype(np.float32)).cuda()
        d_frames = torch.zeros((L.STREAMS, L.FRAMES, 2048), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        enc.encode_frames_device(pcm.data_ptr(), L.FRAMES, d_frames.data_ptr(), asynchronous=True)
        h_out = np.zeros((L.STREAMS, L.FRAMES, 2048), np.uint8)
        enc.write_frames_tonal_ptr(specs.ctypes.data, L.FRAMES, None, recs.ctypes.data, h_out.ctypes.data, B.AT3HIP_ASYNC)
        assert np.array_equal(h_out, want)
        enc.sync()
        queued = d_frames.cpu().numpy()
        enc.reset()
        assert np.array_equal(queued, enc.encode_frames(pcm.cpu().numpy()))
    finally:
        enc.close()


def test_validation_fails_before_anything_is_queued(golden, B):
    """A record outside the contract: AT3HIP_EINVAL naming stream, frame and field, the frames untouched; the context goes on working."""
    nch, specs, flags, _, recs = _case(golden, B, "small_2")
    enc = B.At3pHip(n_streams=L.STREAMS, max_frames=L.FRAMES, channels=nch)
    try:
        bad = recs.copy()
        bad[1, 2]["num_tone_bands"] = 17
        out = np.full((L.STREAMS, L.FRAMES, 2048), 0x5A, np.uint8)
        with pytest.raises(B.At3HipError, match=r"\(-1\).*stream 1, frame 2.*num_tone_bands"):
            enc.write_frames_tonal_ptr(specs.ctypes.data, L.FRAMES, None, bad.ctypes.data, out.ctypes.data, 0)
        assert (out == 0x5A).all()
        assert np.array_equal(enc.write_frames(specs, None, recs), golden["small_2_frames"])
    finally:
        enc.close()


@pytest.mark.parametrize("cid", ["small_1", "share_a_2", "random_2"])
def test_written_frames_decode_with_their_tones(golden, B, cid):
    """At3pHipDecoder(tones=True) takes the written frames without a rejection and gives the restatement's PCM
    (tests/host/at3p_tonal_cpu.c), per stream; without the flag it rejects exactly the frames that carry a block."""
    nch, specs, flags, blocks, recs = _case(golden, B, cid)
    frames = _write(B, nch, specs, flags, recs)
    dec = B.At3pHipDecoder(n_streams=L.STREAMS, channels=nch, max_frames=L.FRAMES)
    try:
        pcm = dec.decode(frames, tones=True)
        assert sum(dec.counters().values()) == 0
        for s in range(L.STREAMS):
            want, rej = T.cpu_tonal_decode(frames[s], nch, tones=True)
            assert rej.sum() == 0
            assert np.array_equal(pcm[s].view(np.uint32), want.view(np.uint32)), s
        dec.reset()
        dec.decode(frames)
        c = dec.counters()
        assert c["tonal_present"] == sum(b is not None for row in blocks for b in row) and sum(c.values()) == c["tonal_present"]
    finally:
        dec.close()
