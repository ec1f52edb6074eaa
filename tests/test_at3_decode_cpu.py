"""The ATRAC3 decoder without a GPU: the C restatement (tests/host/at3_decode_cpu.c) against the goldens, its unpack against
what the encoders decided, call splits, the round trip through the encoder, and the decoder's ABI declarations."""
import ctypes
import os
import re
import subprocess
from collections import Counter

import numpy as np
import pytest

from at3_decode_lib import DELAY, REASONS, ROWS, CpuDecoder, cpu_decode, cpu_lib, unpack
from at3_testlib import ROOT, SIGNALS, oracle, pin_digest

GOLDEN = os.path.join(ROOT, "tests", "golden", "at3_decode.npz")
BFU_START = [0, 8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160, 176, 192, 224, 256, 288, 320, 352, 384, 416, 448, 480,
             512, 576, 640, 704, 768, 896, 1024]
NEW_SYMBOLS = ["at3hip_decoder_create", "at3hip_decoder_destroy", "at3hip_decoder_last_error", "at3hip_decode",
               "at3hip_decoder_sync", "at3hip_decoder_reset", "at3hip_decoder_get_counters", "at3hip_decoder_set_stream"]


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    return g, [str(c) for c in g["cases"]]


def test_restatement_equals_goldens(golden):
    g, names = golden
    assert len(names) >= 80
    seen = np.zeros(len(REASONS), np.int64)
    for name in names:
        fsz, js = (int(v) for v in g[f"{name}_row"])
        pcm, rej = cpu_decode(g[f"{name}_frames"], fsz, js)
        assert np.array_equal(pin_digest(pcm), g[f"{name}_pcm_sha256"]), name
        assert np.array_equal(rej, g[f"{name}_rejected"]), (name, rej, g[f"{name}_rejected"])
        if f"{name}_pcm" in g:
            assert np.array_equal(pcm.view(np.uint32), g[f"{name}_pcm"].view(np.uint32)), name
        seen += rej
    assert (seen > 0).all(), dict(zip(REASONS, seen))   # every rejection reason is pinned


def _check_gains(f, n_points, level, loc, what):
    assert np.array_equal(f["n_points"], n_points), what
    for b in range(4):
        k = int(n_points[b])
        assert np.array_equal(f["level"][b][:k], level[b][:k]) and np.array_equal(f["loc"][b][:k], loc[b][:k]), (what, b)


def _generator():
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_golden_at3_decode", os.path.join(ROOT, "tools", "gen_golden_at3_decode.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def _kept_tonal(t, n_bfu):
    """(position, length, scale factor) of the tapped tonal components whose BFU the frame still codes"""
    return sorted((int(t["tonal_pos"][i]), int(t["tonal_len"][i]), int(t["tonal_sfi"][i])) for i in range(t["n_tonal"])
                  if next(b for b in range(32) if BFU_START[b + 1] > t["tonal_pos"][i]) < n_bfu)


def test_fields_equal_reference_encoder_taps(golden):
    """the unpacked gain points, scale factors and tonal components are the ones the reference encoder decided. The reference's
    tonal position tap is not observable (a pointer into a temporary), so the positions come from the oracle's encode of the
    same input, whose frames and tonal decisions must equal the reference's stored ones"""
    g, names = golden
    gen = _generator()
    n_tonal = n_cases = 0
    for name, br, sig, nch, ng, nt in gen.encoded_cases():
        fsz, js = (int(v) for v in g[f"{name}_row"])
        frames = g[f"{name}_frames"]
        o_frames, o_taps = oracle().encode(SIGNALS[sig](gen.NBLOCKS)[:, :, :nch], br, ng, nt, taps=True)
        assert np.array_equal(o_frames, frames), name
        _, fl = unpack(frames, fsz, js)
        n_cases += 1
        for k in range(fl.shape[0]):
            for c in range(nch):
                f, t, what = fl[k, c], o_taps[k, c], (name, k, c)
                assert f["reason"] == 0, what
                _check_gains(f, g[f"{name}_tap_n_points"][k, c], g[f"{name}_tap_level"][k, c], g[f"{name}_tap_loc"][k, c], what)
                m = f["wl"] > 0
                assert np.array_equal(f["sf"][m], g[f"{name}_tap_sfi"][k, c][m]), what
                nt_ref = int(g[f"{name}_tap_n_tonal"][k, c])
                assert nt_ref == t["n_tonal"], what
                assert sorted(zip(g[f"{name}_tap_tonal_len"][k, c][:nt_ref].tolist(), g[f"{name}_tap_tonal_sfi"][k, c][:nt_ref].tolist())) == \
                    sorted(zip(t["tonal_len"][:nt_ref].tolist(), t["tonal_sfi"][:nt_ref].tolist())), what
                got = sorted((int(f["tonal_pos"][i]), int(f["tonal_len"][i]), int(f["tonal_sf"][i])) for i in range(f["n_tonal"]))
                assert got == _kept_tonal(t, f["n_bfu"]), what   # every kept component, none more
                n_tonal += int(f["n_tonal"])
    assert n_tonal > 0 and n_cases == sum(1 for n in names if f"{n}_tap_n_points" in g)


@pytest.mark.parametrize("row", ROWS, ids=[str(r[1]) for r in ROWS])
@pytest.mark.parametrize("opts", [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 8)], ids=["gain_tonal", "no_gain", "no_tonal", "bfu8"])
def test_fields_equal_oracle_taps(row, opts):
    br, fsz, js = row
    ng, nt, bfu = opts
    for sig, nch in (("burst", 2), ("tones", 2), ("mix", 1)):
        pcm = SIGNALS[sig](6)[:, :, :nch]
        frames, taps = oracle().encode(pcm, br, ng, nt, bfu, taps=True)
        _, fl = unpack(frames, fsz, js)
        for k in range(fl.shape[0]):
            for c in range(nch):
                f, t, what = fl[k, c], taps[k, c], (sig, k, c)
                assert f["reason"] == 0, what
                _check_gains(f, t["n_points"], t["level"], t["loc"], what)
                m = f["wl"] > 0
                assert np.array_equal(f["sf"][m], t["sfi"][m]), what
                if bfu:
                    assert f["n_bfu"] == bfu, what
                got = sorted((int(f["tonal_pos"][i]), int(f["tonal_len"][i]), int(f["tonal_sf"][i])) for i in range(f["n_tonal"]))
                assert got == _kept_tonal(t, f["n_bfu"]), what
                if nt:
                    assert f["n_tonal"] == 0, what
        if js and nch == 1:   # the empty second element of a mono joint-stereo frame parses as a unit with nothing in it
            assert (fl[:, 1]["reason"] == 0).all() and (fl[:, 1]["n_bfu"] >= 1).all() and (fl[:, 1]["wl"] == 0).all()


@pytest.mark.parametrize("row", [ROWS[0], ROWS[3]], ids=["192", "384"])
def test_restatement_in_pieces(golden, row):
    br, fsz, js = row
    g, _ = golden
    frames = np.concatenate([g[f"mix_{fsz}_ch2_frames"], g[f"crafted_{fsz}_frames"], g[f"burst_{fsz}_ch2_frames"]])
    whole, rej = cpu_decode(frames, fsz, js)
    rng = np.random.default_rng(fsz)
    for _ in range(3):
        d = CpuDecoder(fsz, js)
        cuts = np.sort(rng.choice(np.arange(1, len(frames)), 4, replace=False))
        parts = [d.decode(p) for p in np.split(frames, cuts)]
        assert np.array_equal(np.concatenate(parts).view(np.uint32), whole.view(np.uint32))
        assert np.array_equal(d.rejected.astype(np.int64), rej)
        d.reset()
        assert np.array_equal(d.decode(frames).view(np.uint32), whole.view(np.uint32))


def test_generator_reproduces_goldens(golden):
    from at3_decode_lib import have_ref_back_half, ref_back_half
    if not have_ref_back_half():
        pytest.skip("needs oracle/_ref and the reference sources")
    gen = _generator()
    g, names = golden
    got = []
    for name, fsz, js, frames, taps in gen.cases():
        got.append(name)
        assert np.array_equal(frames, g[f"{name}_frames"]), name
        pcm, rej, _ = ref_back_half(frames, fsz, js)
        assert np.array_equal(pin_digest(pcm), g[f"{name}_pcm_sha256"]), name
        assert np.array_equal(rej, g[f"{name}_rejected"]), name
        for k, v in (taps or {}).items():
            assert np.array_equal(v, g[f"{name}_tap_{k}"]), (name, k)
    assert got == names


def _snr(x, y):
    """SNR in dB of decoded y [N][1024][2] against the encoder's input x, aligned by the codec delay (first frame skipped)"""
    x, y = x.reshape(-1, 2), y.reshape(-1, 2)
    n = len(y) - DELAY
    a, b = x[1024:n], y[DELAY + 1024:DELAY + n]
    return 10 * np.log10(np.sum(a.astype(np.float64) ** 2) / np.sum((a.astype(np.float64) - b) ** 2))


# measured on the restatement (16 blocks, oracle-encoded) minus a 2 dB margin: mix, burst, tones
SNR_FLOOR = {192: (0.7, 20.1, 7.3), 272: (1.6, 19.2, 8.2), 304: (1.7, 21.3, 31.7), 384: (2.9, 22.7, 31.9), 424: (3.4, 23.1, 31.9),
             512: (5.3, 24.2, 31.9), 768: (8.5, 28.7, 31.9), 1024: (14.3, 29.4, 31.9)}


def test_round_trip_delay():
    """the end-to-end delay of encoder + decoder: the lag with the best match, for every row"""
    for br, fsz, js in ROWS:
        pcm = SIGNALS["tones"](10)
        out, _ = cpu_decode(oracle().encode(pcm, br)[0], fsz, js)
        x, y = pcm.reshape(-1, 2)[2048:6144, 0], out.reshape(-1, 2)[:, 0]
        err = [np.sum((x - y[2048 + d:6144 + d]) ** 2) for d in range(1000, 1300)]
        assert 1000 + int(np.argmin(err)) == DELAY == 1162


@pytest.mark.parametrize("row", ROWS, ids=[str(r[1]) for r in ROWS])
def test_round_trip_snr(row):
    br, fsz, js = row
    for sig, floor in zip(("mix", "burst", "tones"), SNR_FLOOR[fsz]):
        pcm = SIGNALS[sig](16)
        out, rej = cpu_decode(oracle().encode(pcm, br)[0], fsz, js)
        assert rej.sum() == 0
        assert _snr(pcm, out) >= floor, (sig, _snr(pcm, out))


def test_gain_pairing_on_burst():
    """Demodulate(gains of frame n-1, gains of frame n) is the pairing that inverts the encoder's gain control: the other one
    loses more than 20 dB on the gain-controlled burst signal"""
    lib = cpu_lib()
    lib.at3d_test_reverse_gain_pairing.argtypes = [ctypes.c_int]
    for br, fsz, js in (ROWS[0], ROWS[3]):
        pcm = SIGNALS["burst"](16)
        frames, taps = oracle().encode(pcm, br, taps=True)
        assert taps["n_points"].sum() > 0
        right = _snr(pcm, cpu_decode(frames, fsz, js)[0])
        lib.at3d_test_reverse_gain_pairing(1)
        try:
            wrong = _snr(pcm, cpu_decode(frames, fsz, js)[0])
        finally:
            lib.at3d_test_reverse_gain_pairing(0)
        assert right > 20 and right - wrong > 20, (right, wrong)


def test_decoder_symbols_declared_and_exported():
    from atracdenc_amd import binding
    hdr = open(os.path.join(ROOT, "include", "at3hip.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % s, hdr), s
        assert s in binding.SYMBOLS, s
    assert "#define AT3HIP_DECODE_S16 8u" in hdr and binding.AT3HIP_DECODE_S16 == 8
    if not os.path.exists(binding.LIB_PATH):
        pytest.skip("library not built")
    out = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for s in NEW_SYMBOLS:
        assert s in syms, s
    assert all(s.startswith(("at3hip_", "at1hip_", "at3phip_")) for s in syms), sorted(syms)


def _cli(*args):
    exe = os.path.join(ROOT, "atracdenc_amd", "at3hipenc")
    if not os.path.exists(exe):
        pytest.fail("at3hipenc not built: run __graft_entry__.build()")
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)


def test_cli_at3_decode_argument_errors(tmp_path):
    """`-d` picks the ATRAC3 path by content; ATRAC3plus, headerless ATRAC3 and unsupported rows are refused; anything else
    still reaches the AEA path with its messages"""
    from at3_decode_lib import oma_bytes, riff_at3_bytes
    out = str(tmp_path / "x.wav")
    frames = np.zeros((3, 384), np.uint8)
    r = _cli("-d", "-o", out)
    assert r.returncode == 1 and "at3hipenc -d -i in.aea -o out.wav" in r.stderr and "in.{oma|at3|wav}" in r.stderr
    cases = [
        ("plus.oma", oma_bytes(np.zeros((2, 1024), np.uint8), 1024, False, codec_id=1), "Fatal error: ATRAC3plus decoding is not supported"),
        ("other.oma", oma_bytes(frames, 384, False, codec_id=3), "Fatal error: OMA codec id 3 is not ATRAC3"),
        ("plus.wav", riff_at3_bytes(frames, 384, False, tag=0xFFFE), "Fatal error: ATRAC3plus decoding is not supported"),
        ("raw.at3", bytes([0xA0]) + bytes(383), "Fatal error: raw ATRAC3 input is not supported"),
        ("row.oma", oma_bytes(frames, 384, True), "Fatal error: unsupported ATRAC3 frame size 384 with joint stereo"),
        ("row.wav", riff_at3_bytes(np.zeros((2, 200), np.uint8), 200, False), "Fatal error: unsupported ATRAC3 frame size 200"),
        ("nodata.wav", riff_at3_bytes(frames, 384, False, data=False), "Fatal error: RIFF ATRAC3 file without a data chunk"),
        ("pcm.wav", riff_at3_bytes(frames, 384, False, tag=1), "Fatal error: Can't read AEA header"),   # not ATRAC3: the AEA path
    ]
    for name, data, msg in cases:
        p = tmp_path / name
        p.write_bytes(data)
        r = _cli("-d", "-i", str(p), "-o", out, "--nostdout")
        assert r.returncode == 1 and r.stderr.startswith(msg), (name, r.stderr)
    # a valid ATRAC3 file takes the ATRAC3 path (without a GPU the decoder cannot be created)
    for name, data in (("ok.oma", oma_bytes(frames, 384, False)), ("ok.wav", riff_at3_bytes(np.zeros((2, 192), np.uint8), 192, True))):
        p = tmp_path / name
        p.write_bytes(data)
        r = _cli("-d", "-i", str(p), "-o", out)
        fsz = 384 if name == "ok.oma" else 192
        assert f"Codec: ATRAC3, frame size {fsz}" in r.stdout, (name, r.stdout, r.stderr)
        assert r.returncode == 0 or "at3hip_decoder_create failed" in r.stderr, r.stderr
