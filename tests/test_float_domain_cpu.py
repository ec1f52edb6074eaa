"""The CPU side of the float-domain tests (tests/float_domain_lib.py: NaN, infinities, +-FLT_MAX, samples whose squares
overflow f32, subnormals in block 3 of an ordinary stream).

  * the oracles and restatements that tests/test_float_domain_gpu.py compares the GPU with are defined on every pattern:
    tests/host/float_domain_main.c, built with -fsanitize=address,undefined,float-cast-overflow, runs them all as a child
    process and must exit 0 without a report (a float -> int cast of a NaN or of an out-of-range value, which x86 answers
    with INT_MIN and the GPU with 0 or a saturated value, is a report);
  * what the limiter's and the tone analysis' restatements give on the patterns is enough to compare on (streams are limited,
    and not everywhere; the 48-wave budget binds; NaN residuals are followed by finite slots that hold waves), and the
    sentences of their headers about NaN and infinite samples that can be read off a restatement's output hold;
  * where the reference build exists (oracle/_ref), the oracle equals the real reference on every pattern: ATRAC3 at LP2
    and LP4 and ATRAC1. The reference runs in a child process, twice per setting.

The kernel sources run the same patterns in the `domain` cases of tests/test_*_simt_harness.py.
"""
import concurrent.futures
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import float_domain_lib as FD
from at3_testlib import at1_oracle_encode, have_ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SOURCES = [os.path.join(HERE, "host", "float_domain_main.c"), os.path.join(HERE, "host", "resample_cpu.c"),
           os.path.join(HERE, "host", "loudness_cpu.c"), os.path.join(HERE, "host", "limiter_cpu.c"),
           os.path.join(HERE, "host", "at3p_gha_cpu.c")] + [os.path.join(ROOT, "oracle", n) for n in
                                                             ("at3_oracle.c", "at1_oracle.c", "at3p_oracle.c", "at3p_frame_oracle.c")]
SANITIZE = "-fsanitize=address,undefined,float-cast-overflow"


def test_pattern_table():
    """what the issue's table says of each pattern holds for the arrays the tests use"""
    clean = FD.stream("clean")
    for name in FD.NAMES:
        x = FD.stream(name)
        same = x.view(np.uint32) == clean.view(np.uint32)
        assert same[:FD.BAD_BLOCK].all() and same[FD.BAD_BLOCK + 1:].all(), name   # only block 3 is rewritten
        assert same.all() == (name == "clean")
    b = {n: FD.stream(n)[FD.BAD_BLOCK] for n in FD.NAMES}
    for n in ("max1", "max_alt", "e19_alt", "e15", "subnormal", "clean"):
        assert np.isfinite(b[n]).all(), n
    assert np.isnan(b["nan1"]).sum() == 1 and np.isnan(b["nan_block"]).all()
    assert np.isposinf(b["inf_pair"]).sum() == 1 and np.isneginf(b["inf_pair"]).sum() == 1
    assert np.isposinf(b["inf_left"][:, 0]).all() and np.isfinite(b["inf_left"][:, 1]).all()
    assert set(b["nan_bits"].view(np.uint32).ravel().tolist()) >= {0x7FA00000, 0xFFC00001, 0x7FFFFFFF}
    assert (np.abs(b["max_alt"]) == FD.FLT_MAX).all() and (b["max1"] == FD.FLT_MAX).sum() == 1
    sub = b["subnormal"]
    assert (np.abs(sub) < np.finfo(np.float32).tiny).all() and (sub.view(np.uint32) == 0x80000000).any() and (sub != 0).any()
    assert np.isneginf(b["mixed"]).any() and np.isnan(b["mixed"]).any() and np.isfinite(b["mixed"]).any()
    with np.errstate(over="ignore"):
        e = b["e19_alt"][:, 0]   # 1e38 a square: four of them pass FLT_MAX, the f64 sum of all 1024 is 1e41
        assert np.isinf((e[:4] * e[:4]).sum(dtype=np.float32)) and np.isfinite((e.astype(np.float64) ** 2).sum())
        assert np.isfinite((b["e15"] * b["e15"]).sum(dtype=np.float32))


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_oracles_and_restatements_sanitized(tmp_path):
    exe = str(tmp_path / "float_domain_main")
    subprocess.check_call(["gcc", "-std=gnu11", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fno-fast-math", SANITIZE,
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, *SOURCES, "-lm"])
    data = str(tmp_path / "patterns.bin")
    with open(data, "wb") as f:
        f.write(np.array([len(FD.NAMES), FD.N_BLOCKS, FD.METER_T], np.int32).tobytes())
        for name in FD.NAMES:
            f.write(name.encode().ljust(16, b"\0"))
            f.write(FD.stream(name).tobytes())
            f.write(FD.flat_batch(2, FD.METER_T, (name,))[0].tobytes())
    # (the runtimes are linked statically: the program is sanitized whatever else the process environment loads)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, data], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert f"FLOAT DOMAIN OK: {len(FD.NAMES)} patterns" in r.stdout
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
@pytest.mark.parametrize("nch", [1, 2], ids=["mono", "stereo"])
def test_limiter_restatement_properties(nch):
    """What tests/host/limiter_cpu.c gives on the patterns, from the restatement alone: the comparisons of the harness and of the
    GPU with it are not vacuous (streams are limited, and not everywhere; NaNs reach the output), and the sentences of step 8 of
    include/at3hip_loudness.h that can be read off the output hold."""
    import limiter_lib as LM
    xs = FD.flat_batch(nch, FD.LIMITER_T)
    ix = {n: i for i, n in enumerate(FD.NAMES)}
    T, at = FD.LIMITER_T, FD.BAD_BLOCK * 1024 + 500   # (_nan1, _inf_pair and _max1 write sample 500 of the block, channel 0)

    def run(name, g, c, tp):
        return LM.restate(xs[ix[name]], g, c, tp)

    def stats(g, c, tp):
        return {n: run(n, g, c, tp)[3] for n in FD.NAMES}

    def nans(name, g, c, tp):
        return int(np.isnan(run(name, g, c, tp)[0]).sum())

    c1 = FD.LIMITER_CEIL
    for tp in (False, True):
        # g = 2 at -1 dBFS: the ordinary stream is limited about half of the time, an infinity takes S to 0
        st = stats(2.0, c1, tp)
        assert st["clean"][1] == (2935 if tp else 2934) and 0 < st["clean"][0] < LM.FULL, st["clean"]
        assert st["inf_pair"][0] == 0
        # g = 0: e = 0 * inf = NaN, r = 1: nothing is limited, an infinity least of all; inf * 0 is the output's only NaN
        st = stats(0.0, c1, tp)
        assert all(v == (LM.FULL, 0) for v in st.values()), st
        assert nans("inf_pair", 0.0, c1, tp) == 2
        # g = FLT_MAX: every product overflows or nearly so, all outputs are limited; where s is 0 the product is inf * 0
        st = stats(FD.FLT_MAX, c1, tp)
        assert all(v[1] == T for v in st.values()), st
        assert nans("e15", FD.FLT_MAX, c1, tp) == nans("e19_alt", FD.FLT_MAX, c1, tp) == 1024 * nch
        # the ceiling FLT_MAX: only an infinity or 2 * FLT_MAX passes it: inf_pair and max1 with either detector, max_alt, inf_left
        # and mixed with the sample detector at least (the filter turns some of theirs into NaN); 2 * FLT_MAX needs exactly 1 / 2
        st = stats(2.0, FD.FLT_MAX, tp)
        limited = {n for n, v in st.items() if v[1]}
        assert {"inf_pair", "max1"} <= limited <= {"inf_pair", "max1", "max_alt", "inf_left", "mixed"}, limited
        assert tp or len(limited) == 5
        assert st["max1"][0] * 2 == LM.FULL and 0 < st["max1"][1] < T
        # the smallest ceiling limits everything, the smallest gain only where a sample is infinite
        assert all(v[1] == T for v in stats(2.0, FD.TINY, tp).values())
        st = stats(FD.TINY, c1, tp)
        assert st["inf_pair"][0] == 0 and st["clean"] == st["max1"] == st["e15"] == (LM.FULL, 0), st
        # a NaN sample does not limit, whether one or a whole block of them, read by the true-peak filter or not
        assert st["nan1"] == st["nan_block"] == st["nan_bits"] == (LM.FULL, 0), st
    # ... and with the sample detector it leaves S what it is for the ordinary stream, and passes through as the only NaN
    y, S, _, _ = run("nan1", 2.0, c1, False)
    assert np.array_equal(S, run("clean", 2.0, c1, False)[1])
    assert np.isnan(y[at, 0]) and int(np.isnan(y).sum()) == 1
    # the sample detector around an infinity: S = 0 from the sample to the end of the hold, NaN at the sample itself (inf * 0)
    # and +-0 with the input's sign around it
    y, S, _, _ = run("inf_pair", 2.0, c1, False)
    assert S[at - 1] > 0 and (S[at:at + LM.H + 1] == 0).all()
    assert np.isnan(y[at, 0]) and np.isnan(y[at + 2, 0]) and int(np.isnan(y).sum()) == 2
    rest, x = np.ones((LM.H + 1, nch), bool), xs[ix["inf_pair"], at:at + LM.H + 1]
    rest[0, 0] = rest[2, 0] = False
    zeros = y[at:at + LM.H + 1][rest]
    assert (zeros == 0).all() and np.array_equal(np.signbit(zeros), np.signbit(x[rest])) and np.signbit(zeros).any() and not np.signbit(zeros).all()


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
@pytest.mark.parametrize("nch", [1, 2], ids=["mono", "stereo"])
def test_tones_restatement_properties(oracle, nch):
    """What tests/host/at3p_gha_cpu.c gives on the patterns (12 streams x 6 frames, the pattern in frame 1), from the restatement
    alone: waves, envelope points, sharing bits and non-finite residuals are there for the harness and the GPU to be compared on,
    the 48-wave budget binds, the analysis recovers, and a band that holds a NaN gets no wave."""
    import at3p_gha_lib as G
    ix = {n: i for i, n in enumerate(FD.NAMES)}
    non_finite = ("nan1", "inf_pair", "nan_block", "inf_left", "mixed", "nan_bits")
    whole_block = ("nan_block", "inf_left", "mixed")
    bands = [G.pqf_bands(pcm) for pcm in FD.at3p_batch(nch)]
    for gated, shared in FD.tones_modes(nch):
        recs, resid = FD.tones_analysis(nch, gated, shared)
        waves = {n: [G.n_waves(b) for b in recs[i]] for n, i in ix.items()}
        assert waves["clean"] == [nch * k for k in (1, 2, 1, 1, 1, 2)], waves["clean"]
        assert waves["e15"] == [nch, 0, 48, 0, nch, 2 * nch], waves["e15"]           # the frame budget binds
        amp = [sf for row in G.band_waves(recs[ix["e15"], 2], nch) for b in row for _, sf, _ in b]
        assert max(amp) == 63                                                       # AmpSf saturates
        for n in non_finite:
            i = ix[n]
            assert np.isnan(resid[i, 2]).any(), n
            assert np.isnan(resid[i, 3]).any() == (n in whole_block), n
            assert np.isfinite(resid[i, 4:]).all() and waves[n][4:] == [nch, 2 * nch], (n, waves[n])   # the recovery
        if gated:
            pts = [len(G.points(b, nch)) for b in recs[ix["clean"]]]
            assert pts[1] > 0 and pts[3] > 0, pts
        if shared and nch == 2:
            assert all(len(G.shared_bands(b)) > 0 for b in recs[ix["clean"]])
        if shared and nch == 1:
            plain = FD.tones_analysis(nch, gated, False)
            assert recs.tobytes() == plain[0].tobytes() and resid.tobytes() == plain[1].tobytes()   # the flag changes nothing
        # "comparisons with a NaN are false (no candidate, no wave)": slot f is the block of frames f - 1 and f
        holds, beside = 0, 0
        for n, i in ix.items():
            nan = np.isnan(bands[i]).any(axis=3)                                     # [6][C][16]
            for f in range(1, 6):
                got = np.array([[len(b) for b in row] for row in G.band_waves(recs[i, f], nch)])   # [C][16]
                either = nan[f - 1] | nan[f]
                assert not got[either].any(), (n, f, got[either])
                holds += int(either.sum())
                beside += int(either.any() and got.any())
        assert holds > 0 and (beside > 0 or nch == 1)   # (stereo inf_left: channel 1 keeps its waves beside channel 0's NaNs)


@pytest.fixture(scope="module")
def ref_runs(tmp_path_factory):
    """one child process per pattern: {name: (exit status, stderr, path of its .npz)}"""
    d = tmp_path_factory.mktemp("float_domain_ref")

    def run(name):
        out = str(d / f"{name}.npz")
        r = subprocess.run([sys.executable, os.path.join(HERE, "float_domain_lib.py"), name, out], capture_output=True, text=True,
                           timeout=600, cwd=HERE)
        return r.returncode, r.stderr, out
    with concurrent.futures.ThreadPoolExecutor(max_workers=4) as pool:
        return dict(zip(FD.NAMES, pool.map(run, FD.NAMES)))


@pytest.mark.skipif(not have_ref(), reason="oracle/_ref not built")
@pytest.mark.parametrize("name", FD.NAMES)
def test_oracle_equals_reference(oracle, ref_runs, name):
    """ATRAC3 at LP2 and LP4 (every tool, and none) and ATRAC1 (auto and short windows): the oracle's bytes are the
    reference's. A pattern on which the reference itself crashes or differs between two runs is a finding about the
    pattern (float_domain_lib.REF_UNDEFINED, with an entry in EXCEPTIONS), not something the oracle can be compared with."""
    rc, err, path = ref_runs[name]
    if name in FD.REF_UNDEFINED:
        assert any(p == name for _, p in FD.EXCEPTIONS) and name not in FD.COMPULSORY
        return
    assert rc == 0, f"the reference's encode of {name} ended with status {rc}: {err[-2000:]}"
    g = np.load(path)
    pcm = FD.stream(name)
    for br, ng, nt in FD.REF_AT3:
        a, b = g[f"at3_{br}_{ng}{nt}_0"], g[f"at3_{br}_{ng}{nt}_1"]
        assert np.array_equal(a, b), f"the reference's own frames differ between two runs ({br}, {ng}, {nt})"
        got = oracle.encode(pcm, br, ng, nt)[0]
        bad = np.nonzero((got != a).any(axis=1))[0]
        assert bad.size == 0, f"ATRAC3 {br} no_gain={ng} no_tonal={nt}: frames {bad.tolist()} differ from the reference's"
    for mode, nch in FD.REF_AT1:
        a, b = g[f"at1_{mode}_{nch}_0"], g[f"at1_{mode}_{nch}_1"]
        assert np.array_equal(a, b), f"the reference's own sound units differ between two runs ({mode}, {nch})"
        got = at1_oracle_encode(FD.at1_batch(nch, (name,))[0], mode)
        bad = np.argwhere((got != a).any(axis=2))
        assert bad.size == 0, f"ATRAC1 {mode} ch{nch}: units {bad[:8].tolist()} differ from the reference's"
