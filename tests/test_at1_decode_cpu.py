"""ATRAC1 decoder, host side: the C restatement (tests/host/at1_decode_cpu.c) against the real reference decoder's goldens,
its carried state, the decoder's C ABI surface and the command line's argument errors. No GPU needed."""
import os
import re
import subprocess

import numpy as np
import pytest

import atracdenc_amd
from at1_decode_lib import CpuDecoder, cpu_lib, write_aea
from at3_testlib import ROOT, have_ref, pin_digest

GOLDEN = os.path.join(ROOT, "tests", "golden", "at1_decode.npz")
CLI = os.path.join(ROOT, "atracdenc_amd", "at3hipenc")


@pytest.fixture(scope="session")
def cpu(tmp_path_factory):
    return cpu_lib(str(tmp_path_factory.mktemp("at1_decode_cpu")))


@pytest.fixture(scope="session")
def golden():
    return np.load(GOLDEN)


def test_golden_covers_the_rejections_and_the_clamp(golden):
    names = list(golden["cases"])
    assert len(names) >= 30 and any(n.endswith("_ch1_auto") for n in names) and any(n.endswith("_ch2_auto") for n in names)
    rej = sum(golden[f"{n}_rejected"] for n in names)
    assert rej[0] > 0 and rej[1] > 0, rej
    full = [n for n in names if f"{n}_pcm" in golden.files]
    assert full and any((np.abs(golden[f"{n}_pcm"]) == 1.0).any() for n in full)
    assert all(golden[f"{n}_pcm_sha256"].shape == (32,) for n in names)
    # two- and four-block windows (LogCount 1 / 2 of the low and middle band, 1 / 2 of the high band) are in the inputs
    modes = np.concatenate([golden[f"{n}_units"][..., 0].ravel() for n in names if n.startswith("mixed")])
    assert ((modes >> 6) == 1).any() and ((modes >> 2) & 3 == 2).any()


def test_restatement_equals_reference_goldens(cpu, golden):
    for name in golden["cases"]:
        units = golden[f"{name}_units"]
        d = CpuDecoder(units.shape[1], cpu)
        got = d.decode(units)
        if f"{name}_pcm" in golden.files:
            exp = golden[f"{name}_pcm"]
            assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), (name, int((got.view(np.uint32) != exp.view(np.uint32)).sum()))
        assert np.array_equal(pin_digest(got), golden[f"{name}_pcm_sha256"]), name
        assert d.rejected.tolist() == golden[f"{name}_rejected"].tolist(), name


def _long_stream(golden, nch):
    return np.concatenate([golden[f"{n}_units"] for n in golden["cases"] if f"_ch{nch}" in n])


@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("split", [1, 7, 64])
def test_restatement_in_pieces_equals_one_shot(cpu, golden, nch, split):
    units = _long_stream(golden, nch)
    assert units.shape[0] > 2 * 64
    one = CpuDecoder(nch, cpu)
    exp = one.decode(units)
    d = CpuDecoder(nch, cpu)
    got = np.concatenate([d.decode(units[i:i + split]) for i in range(0, units.shape[0], split)])
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    assert d.rejected.tolist() == one.rejected.tolist()
    d.reset()
    assert np.array_equal(d.decode(units[:5]).view(np.uint32), exp[:5].view(np.uint32))


@pytest.mark.skipif(not have_ref(), reason="needs the reference build oracle/_ref (build container only)")
def test_generator_reproduces_the_goldens(golden, tmp_path):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_golden_at1_decode as gen
    from at1_decode_lib import ref_decode
    for name, units in gen.cases():
        seq, pcm, reasons = ref_decode(np.ascontiguousarray(units))
        assert np.array_equal(seq, golden[f"{name}_units"]), name
        assert np.array_equal(pin_digest(pcm), golden[f"{name}_pcm_sha256"]), name
        if f"{name}_pcm" in golden.files:
            assert np.array_equal(pcm.view(np.uint32), golden[f"{name}_pcm"].view(np.uint32)), name
        assert len(reasons) == int(golden[f"{name}_rejected"].sum()), name


DECODER_SYMBOLS = ["at1hip_decoder_create", "at1hip_decoder_destroy", "at1hip_decoder_last_error", "at1hip_decode", "at1hip_decoder_sync",
                   "at1hip_decoder_reset", "at1hip_decoder_get_counters", "at1hip_decoder_set_stream"]


def test_decoder_symbols_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "at1hip.h")).read()
    for name in DECODER_SYMBOLS:
        assert re.search(rf"\b{name}\(", header), name
        assert name in atracdenc_amd.binding.AT1_SYMBOLS
    out = subprocess.check_output(["nm", "-D", "--defined-only", atracdenc_amd.LIB_PATH], text=True)
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert set(DECODER_SYMBOLS) <= names
    assert "#define AT1HIP_DECODE_S16 8u" in header and atracdenc_amd.binding.AT1HIP_DECODE_S16 == 8
    assert atracdenc_amd.binding.AT3HIP_VERSION == (1 << 16) | 6


def _cli(*args):
    if not os.path.exists(CLI):
        pytest.fail("at3hipenc not built: run __graft_entry__.build()")
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=60)


def test_cli_decode_argument_errors(tmp_path):
    r = _cli("-d", "-o", str(tmp_path / "x.wav"))
    assert r.returncode == 1 and "at3hipenc -d -i in.aea -o out.wav" in r.stderr
    r = _cli("-d", "-e", "atrac1", "-i", "a.aea", "-o", "b.wav")
    assert r.returncode == 1 and "usage" in r.stderr
    r = _cli("-d", "-i", str(tmp_path / "missing.aea"), "-o", str(tmp_path / "x.wav"))
    assert r.returncode == 1 and r.stderr.startswith("Fatal error: unable to open input file")
    bad = tmp_path / "bad.aea"
    bad.write_bytes(b"\x01" * 4096)
    r = _cli("-d", "-i", str(bad), "-o", str(tmp_path / "x.wav"), "--nostdout")
    assert r.returncode == 1 and r.stderr.startswith("Fatal error: invalid AEA header")
    short = tmp_path / "short.aea"
    short.write_bytes(b"\x00\x08" + b"\x00" * 100)
    r = _cli("-d", "-i", str(short), "-o", str(tmp_path / "x.wav"))
    assert r.returncode == 1 and r.stderr.startswith("Fatal error: Can't read AEA header")
    zero = tmp_path / "zero.aea"
    write_aea(str(zero), np.zeros((9, 1, 212), np.uint8))
    data = bytearray(zero.read_bytes())
    data[264] = 0
    zero.write_bytes(bytes(data))
    r = _cli("-d", "-i", str(zero), "-o", str(tmp_path / "x.wav"))
    assert r.returncode == 1 and "no channels" in r.stderr
