"""The gated ATRAC3plus tone analysis on the GPU (include/at3phip.h, FINDING TONES, GATES): at3phip_analyse_tones and
at3phip_encode_frames_tonal(_short) with AT3PHIP_TONES_GATED against the C restatement tests/host/at3p_gha_cpu.c, bit for bit:
three different streams side by side, host and device buffers, one call against per-frame calls, queued against waiting; and
the unflagged calls of the same context against the golden of the ungated analysis."""
import hashlib
import os

import numpy as np
import pytest

import at3p_gha_lib as G

pytestmark = pytest.mark.gpu

NF = 6
NAMES = ("onset", "burst", "noise")   # one call's streams: a gate in one must leave its neighbours' bytes alone


@pytest.fixture(scope="module")
def B():
    from atracdenc_amd import binding
    for name in G.NEW_SYMBOLS + ("at3phip_host_tone_gates",):   # a library without the gates fails every test here
        binding._need(binding.load_library(), name)
    return binding


_cache = {}


def _bands_case(nch):
    """(bands [3][NF][C][16][128], per stream the restatement's (blocks, residual)): the crafted onset at cell 16 as subband input"""
    if ("bands", nch) not in _cache:
        bands = np.stack([G.onset_bands(16, nch, NF), G.pqf_bands(G.signal_pcm("burst", NF, nch)), G.pqf_bands(G.signal_pcm("noise", NF, nch))])
        _cache[("bands", nch)] = (bands, [G.CpuToneAnalyser(nch, True).analyse(bands[s]) for s in range(3)])
    return _cache[("bands", nch)]


def _pcm_case(B, nch):
    """(pcm [3][NF][2048][C] as the 16-bit call widens it, its int16, per stream the restatement pipeline's frames); the onset
    stream is a 3 kHz sine that starts inside frame 2"""
    if ("pcm", nch) not in _cache:
        pcm = np.stack([G.onset_pcm(NF, nch), G.signal_pcm("burst", NF, nch), G.signal_pcm("noise", NF, nch)])
        s16 = np.round(pcm * 32767.0).astype(np.int16)
        pcm = (s16.astype(np.float32) / np.float32(32768.0)).astype(np.float32)
        enc = B.At3pHip(n_streams=1, max_frames=NF, channels=nch)
        try:
            write = lambda specs, recs: enc.write_frames(specs[None], None, recs[None])[0]
            want = [G.pipeline(pcm[s], True, False, write) for s in range(3)]
        finally:
            enc.close()
        assert sum(len(G.points(b, nch)) for b in want[0][1]) > 0 and sum(G.n_waves(b) for b in want[0][1]) > 0
        _cache[("pcm", nch)] = (pcm, s16, np.stack([w[0] for w in want]))
    return _cache[("pcm", nch)]


@pytest.mark.parametrize("nch", [1, 2])
def test_analyse_tones_gated_equals_restatement(B, nch):
    """records and residuals: host buffers in one call and in per-frame calls, then device buffers"""
    import torch
    bands, want = _bands_case(nch)
    enc = B.At3pHip(n_streams=3, max_frames=NF, channels=nch)
    try:
        blocks, resid = enc.analyse_tones(bands, gated=True)
        enc.reset()
        per = [enc.analyse_tones(bands[:, f:f + 1], gated=True) for f in range(NF)]
        enc.reset()
        d_bands = torch.from_numpy(bands).cuda()
        d_res = torch.zeros_like(d_bands)
        torch.cuda.synchronize()
        d_blocks = enc.analyse_tones_device(d_bands.data_ptr(), NF, d_res.data_ptr(), gated=True)
        d_resid = d_res.cpu().numpy()
    finally:
        enc.close()
    for s, name in enumerate(NAMES):
        wb, wr = want[s]
        for how, b, r in (("one call", blocks[s], resid[s]), ("per frame", np.concatenate([p[0][s] for p in per]), np.concatenate([p[1][s] for p in per])),
                          ("device", d_blocks[s], d_resid[s])):
            assert b.tobytes() == wb.tobytes(), (name, how, [G.points(x, nch) for x in b], [G.points(x, nch) for x in wb])
            assert np.array_equal(r.view(np.uint32), wr.view(np.uint32)), (name, how)
    # the crafted onset: the start points of slot 2, and no pre-echo
    assert G.points(blocks[0, 2], nch) == {(ch, b): (17, 0) for ch in range(nch) for b in G.GATE_BANDS}
    assert not resid[0, :3].view(np.uint32).any() and not resid[0, 3, :, :, :64].view(np.uint32).any()
    assert not any(G.points(b, nch) for b in blocks[2])   # noise: no gate


@pytest.mark.parametrize("nch", [1, 2])
def test_encode_frames_tonal_gated_equals_restatement_pipeline(B, nch):
    """frames: float and 16-bit input, host and device buffers, one call against per-frame calls, queued against waiting"""
    import torch
    pcm, s16, exp = _pcm_case(B, nch)
    enc = B.At3pHip(n_streams=3, max_frames=NF, channels=nch)
    got = {}
    try:
        got["float"] = enc.encode_frames_tonal(pcm, gated=True)
        enc.reset()
        got["short"] = enc.encode_frames_tonal_s16(s16, gated=True)
        enc.reset()
        got["per frame"] = np.concatenate([enc.encode_frames_tonal(pcm[:, f:f + 1], gated=True) for f in range(NF)], 1)
        d_pcm, d_s16 = torch.from_numpy(pcm).cuda(), torch.from_numpy(s16).cuda()
        d_parts = [torch.from_numpy(np.ascontiguousarray(pcm[:, a:b])).cuda() for a, b in ((0, 2), (2, 6))]
        d_out = [torch.zeros((3, n, 2048), dtype=torch.uint8, device="cuda") for n in (NF, NF, 2, 4)]
        torch.cuda.synchronize()
        enc.reset()
        enc.encode_frames_tonal_device(d_pcm.data_ptr(), NF, d_out[0].data_ptr(), gated=True)
        got["device"] = d_out[0].cpu().numpy()
        enc.reset()
        enc.encode_frames_tonal_device_s16(d_s16.data_ptr(), NF, d_out[1].data_ptr(), gated=True)
        got["device short"] = d_out[1].cpu().numpy()
        enc.reset()
        for p, o in zip(d_parts, d_out[2:]):   # two queued calls, then one wait
            enc.encode_frames_tonal_device(p.data_ptr(), p.shape[1], o.data_ptr(), asynchronous=True, gated=True)
        enc.sync()
        got["queued"] = np.concatenate([o.cpu().numpy() for o in d_out[2:]], 1)
        enc.reset()
        ungated = enc.encode_frames_tonal(pcm)
    finally:
        enc.close()
    for how, frames in got.items():
        for s, name in enumerate(NAMES):
            bad = (frames[s] != exp[s]).any(axis=1)
            assert not bad.any(), (how, name, np.nonzero(bad)[0].tolist())
    assert (ungated[0] != exp[0]).any() and np.array_equal(ungated[2], exp[2])   # the gate changes the onset stream; noise has none


@pytest.mark.parametrize("nch", [1, 2])
def test_unflagged_calls_on_the_same_context_give_the_golden(B, nch):
    """After flagged calls and a reset the context's unflagged calls are the ungated analysis: the records and the residuals'
    digests of tests/golden/at3p_gha.npz (14 frames of tones, burst and noise) and, in mono, the frames' digests."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "at3p_gha.npz"))
    names, nf = ("tones", "burst", "noise"), int(g["frames"])
    pcm = np.stack([G.signal_pcm(name, nf, nch) for name in names])
    enc = B.At3pHip(n_streams=3, max_frames=nf, channels=nch)
    try:
        bands = enc.pqf(pcm)
        enc.analyse_tones(bands[:, :NF], gated=True)
        enc.encode_frames_tonal(pcm[:, :NF], gated=True)
        enc.reset()
        blocks, resid = enc.analyse_tones(bands)
        enc.reset()
        frames = enc.encode_frames_tonal(pcm)
    finally:
        enc.close()
    for s, name in enumerate(names):
        key = f"{name}_{nch}"
        assert blocks[s].tobytes() == g[key + "_blocks"].tobytes(), key
        assert hashlib.sha256(resid[s].tobytes()).hexdigest() == str(g[key + "_resid_sha256"]), key
        if nch == 1:
            assert hashlib.sha256(frames[s].tobytes()).hexdigest() == str(g[key + "_frames_sha256"]), key
