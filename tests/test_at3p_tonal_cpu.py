"""ATRAC3plus tonal blocks (include/at3phip.h, TONAL BLOCKS) without a GPU: the restatement against the goldens, whose PCM comes
from the reference's own tone synthesis; the host-built tone tables; the new symbol; the kernels' instruction mix."""
import os
import re
import subprocess

import numpy as np
import pytest

import at3p_tonal_lib as L
from at3_testlib import pin_digest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "at3p_tonal.npz")


def golden():
    return np.load(GOLDEN)


def test_restatement_equals_every_tonal_golden():
    g = golden()
    for name in g["cases"]:
        C = int(g[f"{name}_channels"])
        pcm, rej = L.cpu_tonal_decode(g[f"{name}_frames"], C)
        assert np.array_equal(pin_digest(pcm), g[f"{name}_pcm_sha256"]), name
        assert rej.tolist() == g[f"{name}_rejected"].tolist(), name
        _, rej_off = L.cpu_tonal_decode(g[f"{name}_frames"], C, tones=False)
        assert rej_off.tolist() == g[f"{name}_rejected_off"].tolist(), name


def test_goldens_cover_the_rejections_and_the_decoded_frames():
    g = golden()
    tot = sum(g[f"{n}_rejected"] for n in g["cases"])
    assert tot[1] > 0 and tot[3] > 0 and tot[4] > 0 and tot[5] > 0 and tot[2] == 0
    decoded = sum(g[f"{n}_frames"].shape[0] - int(g[f"{n}_rejected"].sum()) for n in g["cases"])
    assert decoded > 100


@pytest.mark.skipif(not L.have_ref_tones(), reason="needs the reference's sources and oracle/_ref")
def test_restatement_equals_the_reference_on_random_blocks():
    rng = np.random.default_rng(7)
    for C in (1, 2):
        frames = np.stack([L.make_tonal_frame(C, L.random_block(rng, C), seed=i) for i in range(10)])
        pcm, rej = L.ref_tonal_back_half(frames, C)
        cpu, crej = L.cpu_tonal_decode(frames, C)
        assert np.array_equal(cpu.view(np.uint32), pcm.view(np.uint32)) and rej.tolist() == crej.tolist()


def test_freq_pack_helper_follows_create_freq_bit_pack():
    # CreateFreqBitPack: ascending after a frequency >= 512 uses GetFirstSetBit(1023 - prev) + 1 bits; descending wins when cheaper
    assert L.freq_pack([5]) == (0, [(5, 10)])
    order, data = L.freq_pack([600, 1000, 1023])
    assert order == 0 and data == [(600, 10), (1000 - (1024 - 512), 9), (1023 - (1024 - 32), 5)]
    order, data = L.freq_pack([1, 2, 4, 8, 16, 900])
    assert order == 1 and data[0] == (900, 10) and data[1] == (16, 10) and data[-1] == (1, 2)


def test_restated_writer_equals_the_reference_written_frames():
    """the refw_* goldens were written by the reference's TAt3PBitStream::WriteFrame with their stored blocks; the restated
    writer spliced into the project's own writer's frame gives the same bytes wherever the unit count is unaffected"""
    import json
    from at3_testlib import at3p_specs, at3p_write_frames
    g = golden()
    compared = 0
    for name in g["cases"]:
        if not str(name).startswith("refw"):
            continue
        C = int(g[f"{name}_channels"])
        blocks = json.loads(str(g[f"{name}_blocks"]))
        ref = g[f"{name}_frames"]
        base = at3p_write_frames(at3p_specs("mix", len(blocks), C, scale=0.5))
        for j, b in enumerate(blocks):
            if b is None:
                assert np.array_equal(base[j], ref[j]), (name, j)
                continue
            if L.n_qu(base[j]) != L.n_qu(ref[j]):
                continue
            assert np.array_equal(L.splice_tonal(base[j], L.tonal_bits(C, b)), ref[j]), (name, j)
            compared += 1
    assert compared >= 80


def test_host_tone_tables_equal_the_fixture_and_the_restatement():
    from atracdenc_amd import binding
    t = binding.at3p_decoder_host_tone_tables()
    g = golden()
    for k in ("sine", "hann", "amp_sf"):
        assert np.array_equal(t[k].view(np.uint32), g[f"host_{k}"].view(np.uint32)), k
    s, h, a = L.tone_tables()
    assert np.array_equal(t["sine"], s) and np.array_equal(t["hann"], h) and np.array_equal(t["amp_sf"], a)
    assert [(int(e) & 0xfff, int(e) >> 12) for e in t["vlc"]] == L.tone_vlc()
    assert binding.load_library().at3phip_decoder_host_tone_tables(None, binding.AT3PHIP_DECODER_TONE_TABLES_BYTES) != 0


def test_new_symbol_is_declared_bound_and_exported():
    from atracdenc_amd import binding
    hdr = open(os.path.join(ROOT, "include", "at3phip.h")).read()
    assert "at3phip_decoder_host_tone_tables(" in hdr and "at3phip_decoder_host_tone_tables" in binding.AT3P_SYMBOLS
    assert "#define AT3PHIP_DECODE_TONES 16u" in hdr and binding.AT3PHIP_DECODE_TONES == 16
    assert f"#define AT3PHIP_DECODER_TONE_TABLES_BYTES {binding.AT3PHIP_DECODER_TONE_TABLES_BYTES}" in hdr
    assert hasattr(binding.load_library(), "at3phip_decoder_host_tone_tables")


def test_tonal_kernels_have_no_fma_division_or_scratch_and_sum_waves_in_double():
    out = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "-fPIC",
                          "--cuda-device-only", "-S", "-o", "-", os.path.join(ROOT, "atracdenc_amd", "csrc", "at3phip.hip")],
                         capture_output=True, text=True, check=True).stdout
    for k in ("k_at3pd_unpack", "k_at3pd_synth", "k_at3pd_state"):
        m = re.search(r"^(_ZN4at3p\d+" + k + r"\w*):[^\n]*\n(.*?)^\.Lfunc_end", out, re.S | re.M)
        assert m, k
        body = m.group(2)
        meta = re.search(r"\.amdhsa_kernel " + re.escape(m.group(1)) + r"\n(.*?)\.end_amdhsa_kernel", out, re.S).group(1)
        assert not re.findall(r"\bv_(?:pk_)?fmac?_\w+", body), k
        assert not re.findall(r"\bv_div_\w+", body), k
        assert not re.findall(r"\bscratch_\w+|\bbuffer_(?:load|store)_\w+", body), k
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", meta), k
    synth = re.search(r"^_ZN4at3p\d+k_at3pd_synth\w*:[^\n]*\n(.*?)^\.Lfunc_end", out, re.S | re.M).group(1)
    # the DCT-IV accounts for 16 f64 multiplies and adds per column; the tone path adds its own
    assert synth.count("v_mul_f64") > 16 and synth.count("v_add_f64") > 16
    assert "v_cvt_f64_f32" in synth and "v_cvt_f32_f64" in synth
