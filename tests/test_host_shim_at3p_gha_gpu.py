"""The C++ mirror's tone analysis on the GPU: the stand-alone program tests/host/test_host_shim_at3p_gha.cpp, which this test is
about, built against libat3hip.so and run once: TAt3PToneAnalyser equals the restatement, and TAt3PEncoder around it and with the
analysis on the device (at3phip_encode_frames_tonal) writes the frames the restatement's pipeline predicts."""
import os
import subprocess

import pytest

import at3p_gha_lib as G


@pytest.mark.gpu
def test_host_cpp_shim_at3p_gha(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe, data = str(tmp_path / "test_host_shim_at3p_gha"), str(tmp_path / "cases.bin")
    libdir = os.path.join(root, "atracdenc_amd")
    n = G.export_shim_cases(data)[0][1]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", os.path.join(root, "tests", "host", "test_host_shim_at3p_gha.cpp"), "-o", exe,
                           f"-L{libdir}", "-lat3hip", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, data], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "HOST SHIM AT3P GHA TEST OK\n" in out.stdout, out.stdout
    assert out.stdout.count(f"{n} records compared, 0 differ; 0 residuals differ") == 2, out.stdout
    assert out.stdout.count(f"{n - 1} frames compared, 0 differ") == 8, out.stdout
