"""ATRAC3plus tonal blocks on the GPU (AT3PHIP_DECODE_TONES): the tonal goldens bit for bit in f32 and s16, the same frames
rejected without the flag, call splits and reset, fuzzed tonal frames against the C restatement, device tensors and queued
calls, and the command line decoding an OMA file of tonal frames."""
import os
import subprocess
import wave

import numpy as np
import pytest

import at3p_tonal_lib as L
from at3_testlib import pin_digest
from at3p_decode_lib import REASONS, oma_bytes

pytestmark = pytest.mark.gpu

GOLDEN = L.GOLDEN


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    return g, [str(c) for c in g["cases"]]


def _dec(nch, n_streams=1, max_frames=64):
    import atracdenc_amd
    return atracdenc_amd.At3pHipDecoder(n_streams=n_streams, channels=nch, max_frames=max_frames, device_id=0)


@pytest.mark.parametrize("nch", [1, 2])
def test_tonal_goldens_bit_identical(golden, nch):
    g, names = golden
    cases, frames = L.side_by_side(g, names, nch)
    dec = _dec(nch, n_streams=len(cases), max_frames=frames.shape[1])
    pcm = dec.decode(frames, tones=True)
    c = dec.counters()
    dec.reset()
    s16 = dec.decode(frames, s16=True, tones=True)
    dec.close()
    want = np.zeros(len(REASONS), np.int64)
    for i, n in enumerate(cases):
        k = g[f"{n}_frames"].shape[0]
        assert np.array_equal(pin_digest(pcm[i, :k]), g[f"{n}_pcm_sha256"]), n
        ref = np.clip(np.rint(pcm[i] * np.float32(32767.0)), -32768, 32767).astype(np.int16)
        assert np.array_equal(s16[i], ref), n
        want += g[f"{n}_rejected"]
    pad = frames.shape[1] * len(cases) - sum(g[f"{n}_frames"].shape[0] for n in cases)   # zero frames: rejected
    want += pad * L.cpu_tonal_decode(np.zeros((1, 2048), np.uint8), nch)[1]
    assert [c[r] for r in REASONS] == want.tolist()


@pytest.mark.parametrize("nch", [1, 2])
def test_without_the_flag_tonal_frames_are_still_rejected(golden, nch):
    g, names = golden
    for n in names:
        if int(g[f"{n}_channels"]) != nch:
            continue
        fr = g[f"{n}_frames"]
        dec = _dec(nch, max_frames=fr.shape[0])
        pcm = dec.decode(fr[None])[0]
        c = dec.counters()
        dec.close()
        assert [c[r] for r in REASONS] == g[f"{n}_rejected_off"].tolist(), n
        want, _ = L.cpu_tonal_decode(fr, nch, tones=False)
        assert np.array_equal(pcm.view(np.uint32), want.view(np.uint32)), n


def test_any_split_and_reset_equal_one_call(golden):
    g, names = golden
    fr = np.concatenate([g["random_2ch_frames"], g["envelopes_2ch_frames"], g["share_mixed_lead1_frames"]])
    n = fr.shape[0]
    dec = _dec(2, max_frames=n)
    whole = dec.decode(fr[None], tones=True)[0]
    want, _ = L.cpu_tonal_decode(fr, 2)
    assert np.array_equal(whole.view(np.uint32), want.view(np.uint32))
    for cut in range(1, n):
        dec.reset()
        a = dec.decode(fr[None, :cut], tones=True)[0]
        b = dec.decode(fr[None, cut:], tones=True)[0]
        assert np.array_equal(np.concatenate([a, b]).view(np.uint32), whole.view(np.uint32)), cut
    dec.reset()
    parts = [dec.decode(fr[None, i:i + 1], tones=True)[0] for i in range(n)]   # one frame per call
    assert np.array_equal(np.concatenate(parts).view(np.uint32), whole.view(np.uint32))
    dec.close()


@pytest.mark.parametrize("nch,streams,nf", [(1, 64, 400), (2, 256, 400)])
def test_fuzzed_tonal_frames_equal_restatement(nch, streams, nf):
    """streams x nf frames drawn from a pool of random tonal blocks, some with flipped bits, some without a tonal block"""
    frames = L.fuzz_tonal_streams(nch, streams, nf)
    dec = _dec(nch, n_streams=streams, max_frames=nf)
    pcm = dec.decode(frames, tones=True)
    c = dec.counters()
    dec.close()
    rej = np.zeros(len(REASONS), np.int64)
    for s in range(streams):
        want, r = L.cpu_tonal_decode(frames[s], nch)
        rej += r
        assert np.array_equal(pcm[s].view(np.uint32), want.view(np.uint32)), s
    assert [c[r] for r in REASONS] == rej.tolist()
    assert rej.sum() < streams * nf // 2


def test_device_tensors_and_async_calls(golden):
    import torch
    g, names = golden
    cases, frames = L.side_by_side(g, names, 2)
    dec = _dec(2, n_streams=len(cases), max_frames=frames.shape[1])
    want = dec.decode(frames, tones=True)
    dec.reset()
    dev = torch.device("cuda", 0)
    fr = torch.from_numpy(frames).to(dev)
    out = torch.empty((len(cases), frames.shape[1], 2048, 2), dtype=torch.float32, device=dev)
    half = frames.shape[1] // 2
    o1 = torch.empty((len(cases), half, 2048, 2), dtype=torch.float32, device=dev)
    o2 = torch.empty((len(cases), frames.shape[1] - half, 2048, 2), dtype=torch.float32, device=dev)
    dec.decode_device(fr[:, :half].contiguous(), o1, asynchronous=True, tones=True)
    dec.decode_device(fr[:, half:].contiguous(), o2, asynchronous=True, tones=True)
    dec.sync()
    out = torch.cat([o1, o2], dim=1)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))
    dec.close()


@pytest.mark.parametrize("nch", [1, 2])
def test_cli_decodes_an_oma_file_of_tonal_frames(tmp_path, golden, nch):
    from atracdenc_amd.binding import LIB_PATH
    g, names = golden
    fr = g[f"random_{nch}ch_frames"]
    assert g[f"random_{nch}ch_rejected"].sum() == 0
    p = tmp_path / "x.oma"
    p.write_bytes(oma_bytes(fr, nch))
    exe = os.path.join(os.path.dirname(LIB_PATH), "at3hipenc")
    r = subprocess.run([exe, "-d", "-i", str(p), "-o", str(tmp_path / "y.wav")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "Skipped" not in r.stderr, r.stderr
    want = np.clip(np.rint(L.cpu_tonal_decode(fr, nch)[0] * np.float32(32767.0)), -32768, 32767).astype(np.int16)
    with wave.open(str(tmp_path / "y.wav")) as w:
        got = np.frombuffer(w.readframes(w.getnframes()), "<i2").reshape(-1, nch)
    assert np.array_equal(got[:want.shape[0] * 2048], want.reshape(-1, nch))
