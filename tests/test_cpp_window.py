"""The C++ host mirror's PhysicalWindowPlan (naive_query_engine_amd/host/naive_db.hpp): tests/cpp/test_window.cpp compiles and links
against the C ABI on the CPU, and runs golden window queries (tests/golden/window_expected.json) on the GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_window")


def build_exe():
    src = os.path.join(ROOT, "tests", "cpp", "test_window.cpp")
    libdir = os.path.join(ROOT, "naive_query_engine_amd")
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", src, "-o", EXE, f"-L{libdir}", "-lnqe_hip", f"-Wl,-rpath,{libdir}",
           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return EXE


def test_cpp_window_compiles_and_links():
    assert os.path.exists(build_exe())


@pytest.mark.gpu
def test_golden_window_queries_through_cpp_host_mirror():
    exe = build_exe()
    out = subprocess.run([exe, os.path.join(ROOT, "tests", "golden")], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "5/5 tests passed" in out.stdout
