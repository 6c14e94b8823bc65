"""NQE_EXPR_STRING_MATCH (quirk Q27) through the host side of expressions (naive_query_engine_amd/csrc/expr_plan.hpp and
string_match_plan.hpp) on the CPU: tests/cpp/test_string_match_plan.cpp includes those headers alone — the node's errors in the order
include/nqe.h states, kind 7 still unknown, the compiled elements, segments and form of the patterns, and that no tree that holds the node
reaches the stack machine or a fused shape."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_string_match_plan(tmp_path):
    exe = str(tmp_path / "test_string_match_plan")
    src = os.path.join(ROOT, "tests", "cpp", "test_string_match_plan.cpp")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-I", os.path.join(ROOT, "naive_query_engine_amd", "csrc"), src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "string match plan ok" in out.stdout, out.stdout + out.stderr
