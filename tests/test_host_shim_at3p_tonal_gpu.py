"""The C++ mirror's analysed ATRAC3plus schedule (TAt3PEncoder with TAt3PSettings and an IAt3PGhaProcessor,
atracdenc_amd/host/at3hip_host.hpp) against the reference's own TAt3PEnc: the stand-alone program
tests/host/test_host_shim_at3p_tonal.cpp, which this test is about, built and run once on the schedule cases of
tests/golden/at3p_tonal_write.npz (UseGha = 0, 1, 5, 7)."""
import os
import subprocess

import numpy as np
import pytest

import at3p_tonal_write_lib as L


@pytest.mark.gpu
def test_host_cpp_shim_at3p_tonal(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe, data = str(tmp_path / "test_host_shim_at3p_tonal"), str(tmp_path / "schedule.bin")
    libdir = os.path.join(root, "atracdenc_amd")
    L.export_schedule(data, np.load(L.GOLDEN))
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(root, "tests", "host", "test_host_shim_at3p_tonal.cpp"), "-o", exe,
                           f"-L{libdir}", "-lat3hip", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, data], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "HOST SHIM AT3P TONAL TEST OK\n" in out.stdout, out.stdout
    assert out.stdout.count("7 frames compared, 0 differ") == 2 * len(L.SCHEDULE_CASES), out.stdout
