"""The hash join on several keys (quirk Q21) in C++.  On the CPU: the probe-side plan (naive_query_engine_amd/csrc/join_keys_plan.hpp —
the range test of a probe key, the code of a probe tuple) is compiled alone with g++ under the address and undefined-behaviour
sanitizers and run, and tests/cpp/test_join_keys.cpp (the host mirror's MultiKeyHashJoin) compiles and links against the C ABI.  On the
GPU that program runs joins over the golden tables; tests/golden/join_keys_expected.json holds the same rows."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_join_keys")


def test_join_keys_plan(tmp_path):
    exe = str(tmp_path / "test_join_keys_plan")
    src = os.path.join(ROOT, "tests", "cpp", "test_join_keys_plan.cpp")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "naive_query_engine_amd", "csrc"), src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "join keys plan ok" in out.stdout, out.stdout + out.stderr


def build_exe():
    src = os.path.join(ROOT, "tests", "cpp", "test_join_keys.cpp")
    libdir = os.path.join(ROOT, "naive_query_engine_amd")
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", src, "-o", EXE, f"-L{libdir}", "-lnqe_hip", f"-Wl,-rpath,{libdir}",
           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return EXE


def test_cpp_join_keys_compiles_and_links():
    assert os.path.exists(build_exe())


@pytest.mark.gpu
def test_joins_on_several_keys_through_cpp_host_mirror():
    exe = build_exe()
    out = subprocess.run([exe, os.path.join(ROOT, "tests", "golden")], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "6/6 tests passed" in out.stdout
