"""The C++ host mirror's PhysicalWindowPlanEx (naive_query_engine_amd/host/naive_db.hpp): tests/cpp/test_window_ex.cpp compiles and links
against the C ABI on the CPU, and runs the golden queries of tests/golden/window_ex_expected.json on the GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_exe(tmp_path):
    exe = str(tmp_path / "test_window_ex")
    src = os.path.join(ROOT, "tests", "cpp", "test_window_ex.cpp")
    libdir = os.path.join(ROOT, "naive_query_engine_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", src, "-o", exe, f"-L{libdir}", "-lnqe_hip", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_window_ex_compiles_and_links(tmp_path):
    assert os.path.exists(build_exe(tmp_path))


@pytest.mark.gpu
def test_golden_window_ex_queries_through_cpp_host_mirror(tmp_path):
    out = subprocess.run([build_exe(tmp_path), os.path.join(ROOT, "tests", "golden")], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "6/6 tests passed" in out.stdout
