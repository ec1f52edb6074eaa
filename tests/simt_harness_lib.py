"""Helpers of the SIMT-harness tests (TEST INFRASTRUCTURE: nothing under atracdenc_amd/ imports this module).

  * build_strict: the strict harness (tools/emu/run_emu.build(strict=True)), built once per test session whichever module asks
    first, and the oracle library that some drivers load.
  * Children: the drivers under tools/emu run as child processes - the harness reads EMU_STRICT, EMU_FENCE, EMU_ORDER and EMU_STREAMS
    when its library loads - several at a time, each on one core, so that the GPU-less suite stays short enough to be run.
  * run_alloc_modes: tests/host/at3p_alloc_modes_main.cpp, the ATRAC3plus engine linked with some of the adaptive writer's units.
"""
import concurrent.futures
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
_built = None


def build_strict():
    """path of the strict harness, compiled on the first call of the session"""
    global _built
    if _built is None:
        sys.path.insert(0, os.path.join(ROOT, "tools", "emu"))
        import run_emu
        run_emu.build(strict=True)
        import at3_testlib
        at3_testlib.oracle()   # compiled here if it is missing: the children would otherwise all start to build it at once
        _built = run_emu.EMU
    return _built


def run_script(script, args, env=None, timeout=900):
    """(exit status, output) of tools/emu/<script> under EMU_STRICT=1 and `env`; a child ended by a signal (a guard page that
    was touched, an abort of the strict checks) has a negative status"""
    e = dict(os.environ, EMU_STRICT="1", OMP_NUM_THREADS="1", **(env or {}))
    for k in ("EMU_FENCE", "EMU_ORDER", "EMU_STREAMS"):
        if k not in (env or {}):
            e.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "emu", script), *args], capture_output=True, text=True,
                       timeout=timeout, env=e, cwd=ROOT)
    return r.returncode, r.stdout + r.stderr


class Children:
    """jobs {name: (script, args, env)} started at once, `workers` at a time in the order given; output(name) waits for one"""

    def __init__(self, jobs, workers=None):
        cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
        self.pool = concurrent.futures.ThreadPoolExecutor(max_workers=workers or max(1, min(8, cores)))
        self.futures = {name: self.pool.submit(run_script, *job) for name, job in jobs.items()}

    def output(self, name):
        rc, out = self.futures[name].result()
        assert rc == 0, f"{name}: exit status {rc}\n{out[-4000:]}"
        return out

    def close(self):
        self.pool.shutdown(wait=True, cancel_futures=True)


def assert_clean(out, min_cases):
    """at least min_cases `bad N` / `mismatching frames N` lines, and every N is 0"""
    counts = re.findall(r"(?:mismatching frames|bad) (\d+)", out)
    assert len(counts) >= min_cases, out[-4000:]
    assert all(c == "0" for c in counts), "\n".join(ln for ln in out.splitlines() if re.search(r"(?:mismatching frames|bad) [1-9]", ln))[-4000:]


ALLOC_MODE_UNITS = {"none": (), "alloc": ("at3p_alloc.hip",), "alloc+sparse": ("at3p_alloc.hip", "at3p_sparse.hip"),
                    "alloc+sparse+rd": ("at3p_alloc.hip", "at3p_sparse.hip", "at3p_rd.hip"),
                    "all": ("at3p_alloc.hip", "at3p_sparse.hip", "at3p_rd.hip", "at3p_psy.hip")}


_alloc_modes = {}


def run_alloc_modes(tmp_path, *configs):
    """tests/host/at3p_alloc_modes_main.cpp in each of `configs`: built with at3phip.hip and the configuration's units, compiled for
    the host with the harness's runtime, run as a child (once per session and configuration), and every check of it held"""
    csrc, emu = os.path.join(ROOT, "atracdenc_amd", "csrc"), os.path.join(ROOT, "tools", "emu")
    for units in configs:
        if units not in _alloc_modes:
            exe = str(tmp_path / ("at3p_alloc_modes_" + units))
            subprocess.check_call([CLANG, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-I", emu, "-include", os.path.join(emu, "at3_pk_emu.hpp"),
                                   "-x", "c++", os.path.join(csrc, "at3phip.hip"), *(os.path.join(csrc, u) for u in ALLOC_MODE_UNITS[units]),
                                   os.path.join(csrc, "at3_tables.cpp"), os.path.join(emu, "emu_runtime.cpp"),
                                   os.path.join(ROOT, "tests", "host", "at3p_alloc_modes_main.cpp"), "-o", exe, "-ldl", "-lpthread"])
            env = {k: v for k, v in os.environ.items() if not k.startswith("EMU_")}
            _alloc_modes[units] = subprocess.run([exe, units], capture_output=True, text=True, env=env, timeout=300)
        r = _alloc_modes[units]
        assert r.returncode == 0 and f"ALLOCATION MODES OK ({units})" in r.stdout, (units, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
