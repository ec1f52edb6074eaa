"""The decoder and resampler kernel SOURCES (at1_decode.hpp, at3_decode.hpp, at3p_decode.hpp with its tonal blocks,
resample.hip), compiled for the host and run lane by lane through the SIMT harness of tools/emu: bit patterns and rejection
counters against the committed goldens and the C restatements under tests/host. Like tests/test_kernels_simt_harness.py for the
encoders, this is the parity gate that exists without a GPU (the `-m gpu` tests are the parity tests proper), and it checks
what a GPU run cannot:

  * EMU_STRICT (every run): a cross-lane read inside divergent control flow aborts; LDS and every device allocation start as
    0xCD bytes.
  * EMU_FENCE=high / low: every device allocation ends (begins) at an inaccessible page, so one word read or written outside a
    buffer ends the child with a signal - with one frame per call on a context of max_frames=1 the frame buffer IS the frame,
    and the frames that the restatement rejects for reading past their end are among those decoded.
  * EMU_ORDER=reverse: the wavefronts of a workgroup run in descending order; a missing __syncthreads() between a producer and
    a consumer wavefront shows in one of the two orders.

Every case is a case of tools/emu/run_emu_decode.py, which runs the engines through the public binding classes with lib_path=
the harness and prints one `bad N` line per comparison. The fuzz inputs are the GPU suite's (the builders of tests/*_lib.py with
the same seeds) plus one larger seeded run per decoder; run_emu_decode.check_share asserts before each comparison that the
restatement accepts at least a quarter of the case's frames and rejects at least one. The environment variables are read when
the harness library loads, so the cases run in child processes, several at a time (simt_harness_lib.Children)."""
import os

import pytest

from simt_harness_lib import CLANG, Children, assert_clean, build_strict

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="needs ROCm's clang++ to compile the kernel sources for the host")

GOLDENS = ["at1_goldens", "at3_goldens", "at3p_goldens", "at3p_tonal_goldens"]
RESAMPLE = ["resample_pairs:0", "resample_pairs:1", "resample_edges"]
SINGLE = ["at1_single", "at3_single", "at3p_single"]
FUZZ_AT3 = ["at3_fuzz:0", "at3_fuzz:1"]
FUZZ_AT3P = ["at3p_fuzz:1", "at3p_fuzz:2"]
CODEBOOK = ["at3p_codebook:1", "at3p_codebook:2", "at3_codebook"]

LARGE = ["at1_fuzz_large:2", "at1_fuzz_large:1", "at3p_fuzz_large:2", "at3p_fuzz_large:1", "at3_fuzz_large:0", "at3_fuzz_large:1"]
FUZZ = ["at1_fuzz:2", "at1_fuzz:1"] + FUZZ_AT3 + FUZZ_AT3P
ENV = {"default": {}, "high": {"EMU_FENCE": "high"}, "low": {"EMU_FENCE": "low"}, "reverse": {"EMU_ORDER": "reverse"}}
# one child per (mode, case), started in this order (the long ones first)
JOBS = ([(m, "at1_fuzz:2") for m in ("default", "reverse")] + [("default", c) for c in LARGE + ["at1_state"]] +
        [(m, c) for c in FUZZ[1:] + GOLDENS + RESAMPLE for m in ("default", "reverse")] +
        [(m, c) for c in GOLDENS + RESAMPLE + SINGLE for m in ("high", "low")] +
        [("default", c) for c in ("at3_state", "at3p_state", "at1_s16", "at3_s16", "at3p_s16")] +
        [(m, "resample_domain") for m in ("high", "low", "reverse")] +
        [(m, c) for c in CODEBOOK for m in ("high", "low", "reverse")])
assert len(set(JOBS)) == len(JOBS)


@pytest.fixture(scope="module")
def children():
    build_strict()
    c = Children({job: ("run_emu_decode.py", ["--nobuild", job[1]], ENV[job[0]]) for job in JOBS})
    yield c
    c.close()


def check(children, mode, case, min_cases):
    """the child of `case` in `mode` ran to its end: at least min_cases comparisons, all of them clean"""
    out = children.output((mode, case))
    assert f"\n{case} done" in out, out[-4000:]
    assert_clean(out, min_cases)
    return out


# ---- 1. goldens ---------------------------------------------------------------------------------------------------------------
# (comparisons per case: PCM and counters per golden case; ATRAC3plus: one per case and the counters of each channel count)
N_GOLDEN = {"at1_goldens": 2 * 38, "at3_goldens": 2 * 83, "at3p_goldens": 28 + 2, "at3p_tonal_goldens": 2 * 46 + 2}


@pytest.mark.parametrize("case", GOLDENS)
def test_goldens_bit_identical(children, case):
    """every case of at1_decode.npz, at3_decode.npz, at3p_decode.npz and (with tones=True, f32 and s16) at3p_tonal.npz"""
    check(children, "default", case, N_GOLDEN[case])


# ---- 2. fuzz against the restatements -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,n", [("at1_fuzz:1", 2), ("at1_fuzz:2", 2), ("at3_fuzz:0", 8), ("at3_fuzz:1", 8), ("at3p_fuzz:1", 6),
                                    ("at3p_fuzz:2", 6)])
def test_fuzz_equals_restatement(children, case, n):
    """The inputs of the GPU suite's test_fuzz_equals_restatement tests, byte for byte (ATRAC1: 6 x 600 units per channel
    count; ATRAC3: 3 x 96 frames per container row and one stream of lightly damaged encoder frames; ATRAC3plus: 4 x 32 frames
    per channel count, without and with tones=True, and tonal-block frames of the GPU suite's pool and seed)."""
    out = check(children, "default", case, n)
    assert out.count("restatement accepts") == n // 2


@pytest.mark.parametrize("case,n", [("at1_fuzz_large:1", 2), ("at1_fuzz_large:2", 2), ("at3_fuzz_large:0", 8), ("at3_fuzz_large:1", 8),
                                    ("at3p_fuzz_large:1", 4), ("at3p_fuzz_large:2", 4)])
def test_larger_fuzz_equals_restatement(children, case, n):
    """Seeds the GPU suite does not have: ATRAC1 4000 mono and 2000 stereo frames; ATRAC3 1344 frames in each of the eight
    rows; ATRAC3plus 1536 frames per channel count without tonal decoding and 2560 tonal-block frames with it."""
    out = check(children, "default", case, n)
    assert out.count("restatement accepts") == n // 2


# ---- 3. carried state ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,n", [("at1_state", 8), ("at3_state", 10), ("at3p_state", 12 + 2 + 19 + 1)])
def test_splits_reset_and_counters(children, case, n):
    """The split patterns of each decoder's test_splits_reset_and_counters, one frame per call and reset() mid-stream: the
    *_state kernels' carried records, and for ATRAC3plus every cut and one frame per call through the tonal goldens (the
    three-record tonal carry)."""
    check(children, "default", case, n)


# ---- 4. s16 output ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,n", [("at1_s16", 3), ("at3_s16", 3), ("at3p_s16", 1)])
def test_s16_output_is_lrintf_of_float(children, case, n):
    check(children, "default", case, n)


# ---- 5. the sample-rate converter ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,n", [("resample_pairs:0", 22), ("resample_pairs:1", 22), ("resample_edges", 6)])
def test_resampler_bit_identical_to_restatement(children, case, n):
    """resample_pairs: all 22 pairs x {1, 2} channels, the four signal kinds of signal(), one call, random cuts plus flush, and
    reset() mid-stream. resample_edges: the max_in = 100 case of test_max_out_and_empty_calls (n_in < K, n_in = 0, flush of an
    empty stream); calls of more than 64 tiles (the driver asserts the count with the launch's own formula); a second call of
    several tiles that begins and ends inside a q, so that tile 0 begins before n0 and the last tile ends after n_end;
    caller-owned buffers of exact size; eleven streams."""
    check(children, "default", case, n)


@pytest.mark.parametrize("mode", ["high", "low", "reverse"])
def test_resampler_float_domain(children, mode):
    """resample_domain: tests/float_domain_lib.py's streams (NaN, infinities, +-FLT_MAX, overflowing and subnormal samples) side
    by side, 48000 <-> 44100, 1 and 2 channels, float and 16-bit output (a NaN gives 0, an infinity +-32767), against the
    restatement of each stream alone: with guard pages on either side of every buffer, and in reversed wavefront order."""
    check(children, mode, "resample_domain", 8)


# ---- 6. guard pages -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fence", ["high", "low"])
@pytest.mark.parametrize("case", GOLDENS + RESAMPLE)
def test_guard_pages_goldens_and_resampler(children, fence, case):
    n = N_GOLDEN.get(case) or {"resample_edges": 6}.get(case, 22)
    check(children, fence, case, n)


@pytest.mark.parametrize("fence", ["high", "low"])
@pytest.mark.parametrize("case,n", [("at1_single", 4), ("at3_single", 16), ("at3p_single", 8)])
def test_guard_pages_one_frame_per_call(children, fence, case, n):
    """Every crafted and random frame of each decoder, one frame per call on a context of max_frames=1. The driver asserts from
    the restatement's counters that frames which read past their end are among them."""
    out = check(children, fence, case, n)
    assert "read past the end)" in out


# ---- 7. reversed wavefront order ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GOLDENS + ["at1_fuzz:1", "at1_fuzz:2"] + FUZZ_AT3 + FUZZ_AT3P + RESAMPLE)
def test_reversed_wavefront_order(children, case):
    n = N_GOLDEN.get(case) or {"resample_edges": 6, "at1_fuzz:1": 2, "at1_fuzz:2": 2, "at3_fuzz:0": 8, "at3_fuzz:1": 8, "at3p_fuzz:1": 6,
                               "at3p_fuzz:2": 6}.get(case, 22)
    check(children, "reverse", case, n)


# ---- 8. every code at every bit phase -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["high", "low", "reverse"])
@pytest.mark.parametrize("case,n", [("at3p_codebook:1", 8), ("at3p_codebook:2", 8), ("at3_codebook", 4)])
def test_codebook_corpus(children, mode, case, n):
    """A slice of the exhaustive code corpora (tests/at3p_decode_lib.code_corpus, tests/at3_decode_lib.code_corpus): every table or
    selector at shifts 0, 7 and 31, with guard pages on either side of every buffer and in both wavefront orders (the guard-page
    runs are in the default order). ATRAC3plus: mono and stereo through the four instantiations of k_at3pd_unpack (plain / sparse
    parse x 2048 bytes / the corpus' frame size), each named in the output; ATRAC3: plain units and joint-stereo frames."""
    out = check(children, mode, case, n)
    if case.startswith("at3p"):
        nch = case[-1]
        sizes = {"1": ("2048", "560"), "2": ("2048", "1488")}[nch]
        for sparse in "01":
            for fb in sizes:
                assert f"at3p codebook ch{nch} sparse={sparse} bytes={fb} (186 frames): bad 0" in out
