"""NQE_EXPR_STRING (quirk Q25) through the host side of expressions (naive_query_engine_amd/csrc/expr_plan.hpp) on the CPU: the node's
errors in their order, result dtypes, nesting, and that a tree with a string step anywhere never becomes a stack-machine program or a
fused shape: tests/cpp/test_string_expr_plan.cpp includes that header alone, is compiled with g++ and run."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_string_expr_plan(tmp_path):
    exe = str(tmp_path / "test_string_expr_plan")
    src = os.path.join(ROOT, "tests", "cpp", "test_string_expr_plan.cpp")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-I", os.path.join(ROOT, "naive_query_engine_amd", "csrc"), src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "string expr plan ok" in out.stdout, out.stdout + out.stderr
