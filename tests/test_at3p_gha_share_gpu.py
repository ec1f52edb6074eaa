"""The ATRAC3plus tone analysis with shared bands on the GPU (include/at3phip.h, FINDING TONES, SHARING): at3phip_analyse_tones and
at3phip_encode_frames_tonal(_short) with AT3PHIP_TONES_SHARED, alone and with AT3PHIP_TONES_GATED, against the C restatement
tests/host/at3p_gha_cpu.c byte for byte: two streams side by side over four frames, in one call and split 1 + 3 with the
state carried, host and device buffers; a mono context; the decoder on the flagged frames; a stream of noise beside a stream of
twin bands. Bytes only: nothing is timed."""
import numpy as np
import pytest

import at3p_gha_lib as G
import at3p_tonal_lib as T

pytestmark = pytest.mark.gpu

NF = 4
SPLIT = ((NF,), (1, 3))
# (the two streams of one call, gated): cases 1 and 2 without gates, cases 2 and 3 (the onset in channel 1 only, then in both) with
CALLS = {"budget+differ": (("budget", "differ"), False), "differ+onset_one": (("differ", "onset_one"), True), "onset_both+budget": (("onset_both", "budget"), True)}


@pytest.fixture(scope="module")
def B():
    from atracdenc_amd import binding
    for name in G.NEW_SYMBOLS + ("at3phip_host_tone_flags",):   # a library without the sharing fails every test here
        binding._need(binding.load_library(), name)
    assert binding.at3p_host_tone_flags() & G.SHARED
    return binding


_cache = {}


def _bands_case(key):
    """(bands [2][NF][2][16][128], per stream the restatement's (blocks, residual))"""
    if ("bands", key) not in _cache:
        names, gated = CALLS[key]
        bands = np.stack([G.CASES[n][0](NF) for n in names])
        _cache[("bands", key)] = (bands, [G.CpuToneAnalyser(2, gated, True).analyse(bands[s]) for s in range(2)])
    return _cache[("bands", key)]


def _case_pcm(name, n):
    """PCM whose subbands behave like the crafted case: budget: three sines in every subband, both channels alike; differ: one of
    subband 5's is stronger in channel 1; onset_*: a 3 kHz sine that starts inside frame 2, in both channels or in channel 1 only
    (channel 0 holds it from the start)"""
    t = np.arange(n * 2048, dtype=np.float64)
    if name in ("budget", "differ"):
        x = np.zeros((2, n * 2048))
        for b in range(16):
            for j in range(3):
                f = (b + (j + 1) / 4.0) * 22050.0 / 16.0
                for c in range(2):
                    amp = 0.018 * (1.5 if (name == "differ" and c == 1 and b == 5 and j == 2) else 1.0)
                    x[c] += amp * np.sin(2 * np.pi * f * t / 44100.0 + 0.37 * (3 * b + j))
    else:
        s = 0.5 * np.sin(2 * np.pi * 3000.0 * t / 44100.0)
        on = s * (t >= 2 * 2048 + 1000)
        x = np.stack([on if name == "onset_both" else s, on])
    return np.ascontiguousarray(x.T.astype(np.float32).reshape(n, 2048, 2))


def _pcm_case(B, key):
    """(pcm [2][NF][2048][2] as the 16-bit call widens it, its int16, per stream the restatement pipeline's (frames, blocks))"""
    if ("pcm", key) not in _cache:
        names, gated = CALLS[key]
        pcm = np.stack([_case_pcm(n, NF) for n in names])
        s16 = np.round(pcm * 32767.0).astype(np.int16)
        pcm = (s16.astype(np.float32) / np.float32(32768.0)).astype(np.float32)
        enc = B.At3pHip(n_streams=1, max_frames=NF, channels=2)
        try:
            write = lambda specs, recs: enc.write_frames(specs[None], None, recs[None])[0]
            want = [G.pipeline(pcm[s], gated, True, write) for s in range(2)]
        finally:
            enc.close()
        _cache[("pcm", key)] = (pcm, s16, np.stack([w[0] for w in want]), [w[1] for w in want])
    return _cache[("pcm", key)]


# ---- 1: the device equals the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(CALLS))
def test_analyse_tones_shared_equals_restatement(B, key):
    """records and residuals: host buffers in one call and split 1 + 3, then device buffers"""
    import torch
    bands, want = _bands_case(key)
    gated = CALLS[key][1]
    enc = B.At3pHip(n_streams=2, max_frames=NF, channels=2)
    got = {}
    try:
        for split in SPLIT:
            enc.reset()
            at, parts = 0, []
            for n in split:
                parts.append(enc.analyse_tones(bands[:, at:at + n], gated=gated, shared=True))
                at += n
            got[f"host {split}"] = (np.concatenate([p[0] for p in parts], 1), np.concatenate([p[1] for p in parts], 1))
        enc.reset()
        d_bands = torch.from_numpy(bands).cuda()
        d_res = torch.zeros_like(d_bands)
        torch.cuda.synchronize()
        d_blocks = enc.analyse_tones_device(d_bands.data_ptr(), NF, d_res.data_ptr(), gated=gated, shared=True)
        got["device"] = (d_blocks, d_res.cpu().numpy())
        enc.reset()
        unflagged = enc.analyse_tones(bands, gated=gated)[0]
    finally:
        enc.close()
    for how, (blocks, resid) in got.items():
        for s, name in enumerate(CALLS[key][0]):
            wb, wr = want[s]
            assert blocks[s].tobytes() == wb.tobytes(), (name, how, [hex(int(x["tone_sharing"])) for x in blocks[s]], [hex(int(x["tone_sharing"])) for x in wb])
            assert np.array_equal(resid[s].view(np.uint32), wr.view(np.uint32)), (name, how)
    assert not unflagged["tone_sharing"].any()
    for s, name in enumerate(CALLS[key][0]):   # what the cases are about
        rec = got["device"][0][s]
        if name == "budget":
            assert int(rec[1]["tone_sharing"]) == 0xffff and G.n_waves(rec[1]) == 48 and not rec[1]["band"][1].tobytes().strip(b"\0")
            assert [len(w) for w in G.band_waves(rec[1], 2)[0]] == [3] * 16
        if name == "differ":
            assert int(rec[1]["tone_sharing"]) == 0xffff & ~(1 << G.DIFFER_BAND) and G.n_waves(rec[1]) == 48
        if name == "onset_one":
            assert G.shared_bands(rec[2]) == [b for b in range(16) if b not in (0, 7, 15)]
        if name == "onset_both":
            assert int(rec[2]["tone_sharing"]) == 0xffff and not rec[2]["band"][1].tobytes().strip(b"\0") and rec[2]["band"][0, 7]["start"] == 17


@pytest.mark.parametrize("key", list(CALLS))
def test_encode_frames_tonal_shared_equals_restatement_pipeline(B, key):
    """frames: float and 16-bit input, host and device buffers, one call against the split 1 + 3"""
    import torch
    pcm, s16, exp, blocks = _pcm_case(B, key)
    gated = CALLS[key][1]
    assert all(sum(len(G.shared_bands(b)) for b in bl) > 0 for bl in blocks)
    enc = B.At3pHip(n_streams=2, max_frames=NF, channels=2)
    got = {}
    try:
        got["float"] = enc.encode_frames_tonal(pcm, gated=gated, shared=True)
        enc.reset()
        got["short"] = enc.encode_frames_tonal_s16(s16, gated=gated, shared=True)
        enc.reset()
        got["split"] = np.concatenate([enc.encode_frames_tonal(pcm[:, :1], gated=gated, shared=True), enc.encode_frames_tonal(pcm[:, 1:], gated=gated, shared=True)], 1)
        enc.reset()
        got["split short"] = np.concatenate([enc.encode_frames_tonal_s16(s16[:, :1], gated=gated, shared=True), enc.encode_frames_tonal_s16(s16[:, 1:], gated=gated, shared=True)], 1)
        d_pcm, d_s16 = torch.from_numpy(pcm).cuda(), torch.from_numpy(s16).cuda()
        d_out = [torch.zeros((2, NF, 2048), dtype=torch.uint8, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        enc.reset()
        enc.encode_frames_tonal_device(d_pcm.data_ptr(), NF, d_out[0].data_ptr(), gated=gated, shared=True)
        got["device"] = d_out[0].cpu().numpy()
        enc.reset()
        enc.encode_frames_tonal_device_s16(d_s16.data_ptr(), NF, d_out[1].data_ptr(), gated=gated, shared=True)
        got["device short"] = d_out[1].cpu().numpy()
        enc.reset()
        unflagged = enc.encode_frames_tonal(pcm, gated=gated)
    finally:
        enc.close()
    for how, frames in got.items():
        for s, name in enumerate(CALLS[key][0]):
            bad = (frames[s] != exp[s]).any(axis=1)
            assert not bad.any(), (how, name, np.nonzero(bad)[0].tolist())
    assert all((unflagged[s] != exp[s]).any() for s in range(2))   # the flag changes every stream here


# ---- 2: mono -----------------------------------------------------------------------------------------------------------------------------
def test_mono_context_ignores_the_flag(B):
    bands = np.ascontiguousarray(np.stack([G.budget_bands(NF)[:, :1], G.stereo_onset_bands(True, NF)[:, :1]]))
    pcm = np.ascontiguousarray(np.stack([_case_pcm("budget", NF)[:, :, :1], _case_pcm("onset_both", NF)[:, :, :1]]))
    enc = B.At3pHip(n_streams=2, max_frames=NF, channels=1)
    try:
        for gated in (False, True):
            out = []
            for shared in (True, False):
                enc.reset()
                blocks, resid = enc.analyse_tones(bands, gated=gated, shared=shared)
                enc.reset()
                out.append((blocks.tobytes(), resid.tobytes(), enc.encode_frames_tonal(pcm, gated=gated, shared=shared).tobytes()))
            assert out[0] == out[1], gated
            assert any(np.frombuffer(out[0][0], G.BLOCK_DTYPE)["num_tone_bands"])
    finally:
        enc.close()


# ---- 3: the device round trip ------------------------------------------------------------------------------------------------------------
def test_flagged_frames_decode_on_the_device_as_on_the_cpu(B):
    """case 1 as PCM (three sines in every subband, both channels alike), 6 frames: the flagged frames through
    At3pHipDecoder(tones=True) equal cpu_tonal_decode bit for bit, with no rejection; every record past the start shares all its
    bands"""
    nf = 6
    pcm = _case_pcm("budget", nf)[None]
    enc = B.At3pHip(n_streams=1, max_frames=nf, channels=2)
    dec = B.At3pHipDecoder(n_streams=1, channels=2, max_frames=nf)
    try:
        frames = enc.encode_frames_tonal(pcm, shared=True)
        enc.reset()
        blocks, _ = enc.analyse_tones(enc.pqf(pcm), shared=True)
        out = dec.decode(frames, tones=True)
        assert sum(dec.counters().values()) == 0
    finally:
        enc.close()
        dec.close()
    assert all(int(b["tone_sharing"]) == (1 << int(b["num_tone_bands"])) - 1 and int(b["num_tone_bands"]) == 16 for b in blocks[0, 1:])
    _, _, rec, why = T.unpack_tonal(frames[0], 2)
    assert not why.any() and rec[2:, 0].all()
    cpu, rej = T.cpu_tonal_decode(frames[0], 2)
    assert rej.sum() == 0
    assert np.array_equal(out[0].view(np.uint32), cpu.view(np.uint32))


# ---- 4: isolation ------------------------------------------------------------------------------------------------------------------------
def test_a_stream_of_noise_beside_twin_bands_is_untouched(B):
    pcm = np.stack([G.signal_pcm("noise", NF, 2), _case_pcm("budget", NF)])
    enc = B.At3pHip(n_streams=2, max_frames=NF, channels=2)
    solo = B.At3pHip(n_streams=1, max_frames=NF, channels=2)
    try:
        frames = enc.encode_frames_tonal(pcm, shared=True)
        enc.reset()
        blocks, _ = enc.analyse_tones(enc.pqf(pcm), shared=True)
        alone = [solo.encode_frames_tonal(pcm[s:s + 1], shared=True)[0] for s in range(2) if solo.reset() or True]
    finally:
        enc.close()
        solo.close()
    assert not blocks[0].tobytes().strip(b"\0") and blocks[1]["tone_sharing"].any()
    assert np.array_equal(frames[0], alone[0]) and np.array_equal(frames[1], alone[1])
