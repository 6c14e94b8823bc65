"""The C++ host mirror's PhysicalDistinctPlan and PhysicalSetOpPlan (naive_query_engine_amd/host/naive_db.hpp): tests/cpp/test_set_ops.cpp
compiles and links against the C ABI on the CPU; on the GPU it runs golden queries (tests/golden/set_ops_expected.json holds the same
rows) and a constructed case whose probes wrap from the end of the set table to its start."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_set_ops")


def build_exe():
    src = os.path.join(ROOT, "tests", "cpp", "test_set_ops.cpp")
    libdir = os.path.join(ROOT, "naive_query_engine_amd")
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", src, "-o", EXE, f"-L{libdir}", "-lnqe_hip", f"-Wl,-rpath,{libdir}",
           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return EXE


def test_cpp_set_ops_compiles_and_links():
    assert os.path.exists(build_exe())


@pytest.mark.gpu
def test_golden_set_op_queries_and_the_wrapping_probe_through_cpp_host_mirror():
    exe = build_exe()
    out = subprocess.run([exe, os.path.join(ROOT, "tests", "golden")], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "6/6 tests passed" in out.stdout
