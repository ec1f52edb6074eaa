"""The CPU side of the float-domain tests (tests/float_domain_lib.py: NaN, infinities, +-FLT_MAX, samples whose squares
overflow f32, subnormals in block 3 of an ordinary stream).

  * the oracles and restatements that tests/test_float_domain_gpu.py compares the GPU with are defined on every pattern:
    tests/host/float_domain_main.c, built with -fsanitize=address,undefined,float-cast-overflow, runs them all as a child
    process and must exit 0 without a report (a float -> int cast of a NaN or of an out-of-range value, which x86 answers
    with INT_MIN and the GPU with 0 or a saturated value, is a report);
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
           os.path.join(HERE, "host", "loudness_cpu.c")] + [os.path.join(ROOT, "oracle", n) for n in
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
