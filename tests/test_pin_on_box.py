"""The oracle's pin, re-verified ON THE MACHINE THAT MEASURES: a slice of test_oracle_vs_ref.py / test_oracle_golden.py
marked `gpu` so that the driver's `-m gpu` run proves, on the GPU box (whose libm builds the product's tables at
at3hip_create), that oracle == the reference's outputs for that slice (tests/golden/pin.npz, written from the reference
build by tools/gen_golden_pin.py) == committed golden vectors, and that the PRODUCT's host-built tables equal the
reference's. The full matrices stay in the CPU suite."""
import numpy as np
import pytest

from at3_testlib import LP2, LP4, PIN_CONTAINER_BFUS, PIN_CONTAINER_ROWS, PIN_OPTION_BLOCKS, PIN_OPTION_SETS, PIN_PATH, TAP_DTYPE, have_ref, \
    pin_outputs, ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pin():
    return np.load(PIN_PATH)


@pytest.fixture(scope="module")
def oracle_pin(oracle, pin):
    return pin_outputs(oracle, pin["flatness_in"], pin["log2f_in"])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def test_pin_inputs_reproduce_and_match_reference(oracle_pin, pin):
    """The PCM the pin's encodes run on is regenerated here bit for bit as the fixture was written from it, and where the
    reference build is present its outputs are still the stored ones."""
    for k in pin.files:
        if k.startswith("pcm_"):
            assert np.array_equal(oracle_pin[k], pin[k]), k
    if have_ref():
        now = pin_outputs(ref(), pin["flatness_in"], pin["log2f_in"])
        for k, v in now.items():
            assert np.array_equal(v, pin[k]), k


def test_oracle_tables_equal_golden(oracle, golden_stages):
    for k, v in oracle.tables().items():
        assert np.array_equal(bits(v), bits(golden_stages[f"table_{k}"])), k


def test_product_tables_equal_golden(golden_stages):
    """at3hip_host_tables = the block at3hip_create uploads, built with THIS host's libm, against the arrays the reference
    wrote into tests/golden/stages.npz (tools/gen_golden.py) and against the oracle's tables for the rest."""
    from atracdenc_amd import binding as B
    t = B.at3_host_tables()
    g = golden_stages
    assert np.array_equal(bits(t["scale"]), bits(g["table_scale"]))
    assert np.array_equal(bits(t["enc_win"]), bits(g["table_encwin"]))
    assert np.array_equal(bits(t["gain_level"]), bits(g["table_gainlevel"]))
    assert np.array_equal(bits(t["gain_interp"][:31]), bits(g["table_gaininterp"]))
    assert np.array_equal(bits(t["qmf_win"]), bits(g["table_qmfwin"]))
    assert np.array_equal(bits(t["loud_curve"]), bits(g["table_loud"]))
    # ATH per BFU (atrac3_bitstream.cpp:694-718): minimum of the per-line thresholds the reference's CalcATH produced
    bfu_start = [0, 8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160, 176, 192, 224, 256, 288, 320, 352, 384, 416, 448, 480, 512,
                 576, 640, 704, 768, 896, 1024]
    ath = g["table_ath"]
    import ctypes
    libm = ctypes.CDLL("libm.so.6")
    libm.pow.restype = ctypes.c_double
    libm.pow.argtypes = [ctypes.c_double, ctypes.c_double]
    exp = np.array([np.float32(libm.pow(10.0, float(np.float32(0.1) * np.float32(min(np.float32(999.0), ath[bfu_start[b]:bfu_start[b + 1]].min())))))
                    for b in range(32)], np.float32)
    assert np.array_equal(bits(t["ath_bfu"]), bits(exp))


@pytest.mark.parametrize("br", [LP2, LP4])
def test_oracle_equals_reference_option_sets(oracle_pin, pin, br):
    """One signal per option set (frames and stage taps), as test_oracle_vs_ref.py::test_frames_and_taps does for all."""
    for name, ng, nt in PIN_OPTION_SETS:
        key = f"opt_{br}_{name}"
        assert np.array_equal(oracle_pin[f"{key}_frames"], pin[f"{key}_frames"]), (name, ng, nt)
        assert pin[f"{key}_frames"].shape[0] == PIN_OPTION_BLOCKS - 1
        for k in TAP_DTYPE.names:
            if k != "tonal_pos":
                assert np.array_equal(oracle_pin[f"{key}_tap_{k}"], pin[f"{key}_tap_{k}"]), (name, k)


def test_oracle_equals_reference_container_rows(oracle_pin, pin):
    for br, fsz in PIN_CONTAINER_ROWS:
        for bfu in PIN_CONTAINER_BFUS:
            fo, fr = oracle_pin[f"row_{br}_bfu{bfu}_frames"], pin[f"row_{br}_bfu{bfu}_frames"]
            assert fo.shape == (15, fsz) and np.array_equal(fo, fr), (br, bfu)
        assert np.array_equal(oracle_pin[f"row_{br}_stress_frames"], pin[f"row_{br}_stress_frames"]), br


def test_oracle_equals_reference_flatness_and_log2f(oracle_pin, pin):
    """The two libm-dependent stage functions (std::log / std::exp in CalcSpectralFlatnessPerBfu, std::log2(float)) on this
    box's libm: oracle (which calls libm for the first and restates the second) against the reference's outputs."""
    assert pin["flatness_in"].shape == (3, 1024) and pin["log2f_in"].shape == (5000,)
    assert np.array_equal(bits(oracle_pin["flatness_out"]), bits(pin["flatness_out"]))
    assert np.array_equal(bits(oracle_pin["log2f_out"]), bits(pin["log2f_out"]))
