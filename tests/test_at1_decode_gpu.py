"""ATRAC1 decoder on the MI355X (include/at1hip.h, atracdenc_amd/csrc/at1_decode.hpp): bit-identical to the real reference
decoder's goldens and to the C restatement (tests/host/at1_decode_cpu.c) on fuzzed units, across call splits, resets, device
buffers, queued calls, 16-bit output, long streams, the encoder round trip and the command line."""
import os
import subprocess

import numpy as np
import pytest

import atracdenc_amd
from atracdenc_amd import At1Hip, At1HipDecoder, At3HipError
from at1_decode_lib import GOLDEN, CpuDecoder, cpu_lib, cpu_ref, fuzz_units, random_modes, read_wav, s16_of, set_block_modes, write_aea
from at3_testlib import ROOT, SIGNALS, at1_blocks, pcm_stress, pin_digest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return cpu_lib(str(tmp_path_factory.mktemp("at1_decode_cpu")))


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_goldens_bit_identical(golden):
    for name in golden["cases"]:
        units = golden[f"{name}_units"]
        dec = At1HipDecoder(n_streams=1, max_frames=units.shape[0], channels=units.shape[1])
        got = dec.decode(units[None])[0]
        c = dec.counters()
        dec.close()
        assert np.array_equal(pin_digest(got), golden[f"{name}_pcm_sha256"]), name
        if f"{name}_pcm" in golden.files:
            assert np.array_equal(bits(got), bits(golden[f"{name}_pcm"])), (name, int((bits(got) != bits(golden[f"{name}_pcm"])).sum()))
        assert [c["bad_block_size"], c["read_past_end"]] == golden[f"{name}_rejected"].tolist(), name


@pytest.mark.parametrize("nch", [1, 2])
def test_fuzz_equals_restatement(cpu, nch):
    units = fuzz_units(nch, 6, 600, seed=40 + nch)
    exp, rej = cpu_ref(cpu, units)
    dec = At1HipDecoder(n_streams=6, max_frames=600, channels=nch)
    got = dec.decode(units)
    c = dec.counters()
    dec.close()
    assert sum(rej) > 100
    assert np.array_equal(bits(got), bits(exp)), int((bits(got) != bits(exp)).sum())
    assert [c["bad_block_size"], c["read_past_end"]] == rej


def test_splits_reset_and_counters(cpu):
    units = fuzz_units(2, 3, 300, seed=7)
    exp, rej = cpu_ref(cpu, units)
    dec = At1HipDecoder(n_streams=3, max_frames=300, channels=2)
    for cuts in ([1, 7, 64, 100, 128], [299, 1], [13] * 23 + [1]):
        dec.reset()
        parts, pos = [], 0
        for n in cuts:
            parts.append(dec.decode(units[:, pos:pos + n]))
            pos += n
        assert pos == 300
        got = np.concatenate(parts, axis=1)
        assert np.array_equal(bits(got), bits(exp)), cuts
        c = dec.counters(reset=True)
        assert [c["bad_block_size"], c["read_past_end"]] == rej
        assert dec.counters() == {"bad_block_size": 0, "read_past_end": 0}
    dec.close()


def test_device_tensors_ordered_and_queued(cpu):
    import torch
    units = fuzz_units(2, 4, 256, seed=9)
    exp, _ = cpu_ref(cpu, units)
    dec = At1HipDecoder(n_streams=4, max_frames=256, channels=2)
    # ordered (default): the units are produced on torch's current stream right before the call
    src = torch.from_numpy(units).cuda()
    u = torch.zeros_like(src)
    out = torch.full((4, 256, 512, 2), float("nan"), device="cuda")
    torch.cuda._sleep(20_000_000)
    u.copy_(src)
    dec.decode_device(u, out)
    assert np.array_equal(bits(out.cpu().numpy()), bits(exp))
    # the same on a side stream of torch's: the call is queued there, behind the copy, and torch's next work follows it
    dec.reset()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        u2 = torch.zeros_like(src)
        out2 = torch.full((4, 256, 512, 2), float("nan"), device="cuda")
        torch.cuda._sleep(20_000_000)
        u2.copy_(src)
        dec.decode_device(u2, out2)
        res = out2.cpu()
    assert np.array_equal(bits(res.numpy()), bits(exp))
    # queued calls: four pieces back to back, one sync
    dec.reset()
    pieces = [(0, 50), (50, 51), (51, 200), (200, 256)]
    ins = [u[:, a:b].contiguous() for a, b in pieces]
    outs = [torch.zeros((4, b - a, 512, 2), device="cuda") for a, b in pieces]
    torch.cuda.synchronize()
    for i, o in zip(ins, outs):
        dec.decode_device(i, o, asynchronous=True)
    dec.sync()
    assert np.array_equal(bits(torch.cat(outs, 1).cpu().numpy()), bits(exp))
    # 16-bit output on the device
    dec.reset()
    o16 = torch.zeros((4, 256, 512, 2), dtype=torch.int16, device="cuda")
    dec.decode_device(u, o16)
    assert np.array_equal(o16.cpu().numpy(), s16_of(exp))
    dec.close()


def test_s16_output_is_lrintf_of_float(golden):
    for name in ("stress_ch2_auto", "crafted_ch1", "mixed_windows_ch2"):
        units = golden[f"{name}_units"][None]
        dec = At1HipDecoder(n_streams=1, max_frames=units.shape[1], channels=units.shape[2])
        f32 = dec.decode(units)
        assert np.array_equal(pin_digest(f32[0]), golden[f"{name}_pcm_sha256"]), name
        dec.reset()
        got = dec.decode(units, s16=True)
        dec.close()
        assert got.dtype == np.int16 and np.array_equal(got, s16_of(f32)), name


def test_long_stream(cpu):
    n = 65536 + 1234
    rng = np.random.default_rng(3)
    g = np.load(GOLDEN)
    pool = np.concatenate([g[f"{c}_units"] for c in g["cases"] if "_ch2" in c])
    units = pool[rng.integers(0, pool.shape[0], n)]
    units = np.where(rng.random((n, 1, 1)) < 0.3, set_block_modes(units, random_modes(units.shape[:2], rng)), units)
    units[40000:40100] = set_block_modes(units[40000:40100], np.tile([1, 1, 2], (100, 2, 1)))   # a long run of two-block frames
    exp, rej = cpu_ref(cpu, units[None])
    dec = At1HipDecoder(n_streams=1, max_frames=40000, channels=2)
    got = np.concatenate([dec.decode(units[None, a:a + 40000]) for a in range(0, n, 40000)], axis=1)
    c = dec.counters()
    dec.close()
    assert np.array_equal(bits(got), bits(exp)), int((bits(got) != bits(exp)).sum())
    assert [c["bad_block_size"], c["read_past_end"]] == rej


def test_bad_arguments():
    with pytest.raises(At3HipError):
        At1HipDecoder(n_streams=1, max_frames=8, channels=3)
    with pytest.raises(At3HipError):
        At1HipDecoder(n_streams=0, max_frames=8, channels=2)
    with pytest.raises(At3HipError):
        At1HipDecoder(n_streams=1, max_frames=0, channels=2)
    with pytest.raises(At3HipError):
        At1HipDecoder(n_streams=40000, max_frames=8, channels=2)
    dec = At1HipDecoder(n_streams=1, max_frames=8, channels=2)
    with pytest.raises(At3HipError):
        dec.decode(np.zeros((1, 9, 2, 212), np.uint8))
    units = np.zeros((1, 2, 2, 212), np.uint8)
    out = np.zeros((1, 2, 512, 2), np.float32)
    lib = dec.lib
    assert lib.at1hip_decode(dec.ctx, units.ctypes.data, 0, out.ctypes.data, 0) == -1
    assert lib.at1hip_decode(dec.ctx, None, 2, out.ctypes.data, 0) == -1
    assert lib.at1hip_decode(dec.ctx, units.ctypes.data, 2, out.ctypes.data, 0x100) == -1
    assert lib.at1hip_decode(None, units.ctypes.data, 2, out.ctypes.data, 0) == -1
    assert lib.at1hip_decoder_get_counters(dec.ctx, None, 0) == -1
    assert lib.at1hip_decoder_sync(None) == -1 and lib.at1hip_decoder_reset(None) == -1
    assert dec.decode(units).shape == (1, 2, 512, 2)   # still usable
    dec.close()


def test_encoder_round_trip(cpu):
    pcm = np.stack([at1_blocks(SIGNALS["mix"](10), 2), at1_blocks(pcm_stress(10), 2)])
    enc = At1Hip(n_streams=2, max_blocks=pcm.shape[1], channels=2)
    units = enc.encode(pcm)
    enc.close()
    dec = At1HipDecoder(n_streams=2, max_frames=units.shape[1], channels=2)
    got = dec.decode(units)
    dec.close()
    exp, rej = cpu_ref(cpu, units)
    assert rej == [0, 0]
    assert np.array_equal(bits(got), bits(exp))


def test_cli_decode(cpu, golden, tmp_path):
    exe = os.path.join(ROOT, "atracdenc_amd", "at3hipenc")
    for name in ("crafted_ch2", "stress_ch1_auto", "mixed_windows_ch2"):
        units = golden[f"{name}_units"]
        pcm = CpuDecoder(units.shape[1], cpu).decode(units)
        assert np.array_equal(pin_digest(pcm), golden[f"{name}_pcm_sha256"]), name   # the reference's samples
        aea, wav = str(tmp_path / f"{name}.aea"), str(tmp_path / f"{name}.wav")
        write_aea(aea, units)
        r = subprocess.run([exe, "-d", "-i", aea, "-o", wav, "--batch", "5"], capture_output=True, text=True, timeout=120)
        n_frames, nch = units.shape[:2]
        calls = max(1, -(-(n_frames - 5) // 8))   # TAeaInput::GetLengthInSamples and the engine's 4096-sample calls
        ok = 8 * calls <= n_frames
        assert r.returncode == (0 if ok else 1), r.stderr
        h, samples = read_wav(wav)
        n = 8 * min(calls, n_frames // 8)
        assert (h["riff"], h["wave"], h["fmt"], h["fmt_len"], h["tag"], h["nch"], h["rate"], h["bits"], h["data"]) == \
               (b"RIFF", b"WAVE", b"fmt ", 16, 1, nch, 44100, 16, b"data")
        assert h["data_len"] == n * 512 * nch * 2 and h["size"] == 36 + h["data_len"] and h["file_len"] == 44 + h["data_len"]
        assert h["byte_rate"] == 44100 * 2 * nch and h["align"] == 2 * nch
        assert np.array_equal(samples.reshape(n, 512, nch), s16_of(pcm[:n])), name
        lines = [ln for ln in r.stderr.splitlines() if ln.startswith("Skipping invalid ATRAC1 frame: ")]
        if ok and n == n_frames:
            assert len(lines) == int(golden[f"{name}_rejected"].sum()), name
