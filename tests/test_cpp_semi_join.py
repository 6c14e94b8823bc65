"""The C++ host mirror's HashSemiJoin (naive_query_engine_amd/host/naive_db.hpp): tests/cpp/test_semi_join.cpp compiles and links
against the C ABI on the CPU, and runs the golden semi / anti joins (tests/golden/semi_join_expected.json) on the GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_semi_join")


def build_exe():
    src = os.path.join(ROOT, "tests", "cpp", "test_semi_join.cpp")
    libdir = os.path.join(ROOT, "naive_query_engine_amd")
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", src, "-o", EXE, f"-L{libdir}", "-lnqe_hip", f"-Wl,-rpath,{libdir}",
           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return EXE


def test_cpp_semi_join_compiles_and_links():
    assert os.path.exists(build_exe())


@pytest.mark.gpu
def test_golden_semi_joins_through_cpp_host_mirror():
    exe = build_exe()
    out = subprocess.run([exe, os.path.join(ROOT, "tests", "golden")], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "5/5 tests passed" in out.stdout
