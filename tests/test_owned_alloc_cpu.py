"""Every engine releases what it allocated, whenever it allocated it: the buffers that the first host-memory call of a kind
makes (16-bit input staging, output staging, the limiter's buffers, the tone analysis, the quant tap, the growing staging of
the ATRAC3 stage-level entry points) live in the engine's own list (at3_host_util.hpp: dev_alloc, destroy_engine), as do
those of a create that fails half-way.

tests/host/owned_alloc_main.cpp is a stand-alone program: the library's sources compiled for the host with the SIMT
harness's runtime (tools/emu), all under -fsanitize=address,undefined with the runtimes linked statically, run as a child
process with leak detection on. Nothing sanitized is loaded into Python."""
import concurrent.futures
import os
import subprocess

import pytest

from simt_harness_lib import CLANG, ROOT

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="needs ROCm's clang++ to compile the host sources")

CSRC = os.path.join(ROOT, "atracdenc_amd", "csrc")
EMU = os.path.join(ROOT, "tools", "emu")
SOURCES = [os.path.join(CSRC, n) for n in ("at3hip.hip", "at1hip.hip", "at3phip.hip", "resample.hip", "loudness.hip", "at3_tables.cpp")] + [
    os.path.join(EMU, "emu_runtime.cpp"), os.path.join(ROOT, "tests", "host", "owned_alloc_main.cpp")]
# (no alignment check: it would judge the kernels, whose paired loads of 4-byte aligned LDS words the GPU allows - this
# program is about the host code's allocations)
FLAGS = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize=alignment",
         "-fno-sanitize-recover=all"]


def test_every_allocation_is_released(tmp_path):
    def compile_one(src):
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        subprocess.check_call([CLANG, *FLAGS, "-ffp-contract=off", "-I", EMU, "-include", os.path.join(EMU, "at3_pk_emu.hpp"), "-x", "c++",
                               "-c", src, "-o", obj])
        return obj
    with concurrent.futures.ThreadPoolExecutor(max_workers=len(SOURCES)) as pool:
        objs = list(pool.map(compile_one, SOURCES))
    exe = str(tmp_path / "owned_alloc_main")
    subprocess.check_call([CLANG, *FLAGS, "-static-libsan", "-o", exe, *objs, "-ldl", "-lpthread"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for k in ("EMU_TRACE", "EMU_FENCE", "EMU_ORDER", "EMU_STRICT"):
        env.pop(k, None)
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "OWNED ALLOCATIONS OK" in r.stdout and r.stdout.count("half-made creates") == 8, r.stdout[-2000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
