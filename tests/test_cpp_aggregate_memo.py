"""The aggregate's plan memo (naive_query_engine_amd/csrc/aggregate_memo.hpp: what a context remembers of a query shape between
executions) on the CPU: tests/cpp/test_aggregate_memo.cpp includes that header alone, is compiled with g++ and run."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_aggregate_memo(tmp_path):
    exe = str(tmp_path / "test_aggregate_memo")
    src = os.path.join(ROOT, "tests", "cpp", "test_aggregate_memo.cpp")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "naive_query_engine_amd", "csrc"), src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "aggregate memo ok" in out.stdout, out.stdout + out.stderr
