"""The host analysis of DISTINCT and the set operators (naive_query_engine_amd/csrc/set_ops_plan.hpp: the argument checks in their
order, the capacity rule, the canonical words and the NULL tag, the instantiation choice) on the CPU: tests/cpp/test_set_ops_plan.cpp
includes that header alone, is compiled with g++ and run."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_set_ops_plan(tmp_path):
    exe = str(tmp_path / "test_set_ops_plan")
    src = os.path.join(ROOT, "tests", "cpp", "test_set_ops_plan.cpp")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-I", os.path.join(ROOT, "naive_query_engine_amd", "csrc"), src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "set ops plan ok" in out.stdout, out.stdout + out.stderr
