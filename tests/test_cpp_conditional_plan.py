"""NQE_EXPR_CONDITIONAL (quirk Q28) through the host side of expressions (naive_query_engine_amd/csrc/expr_plan.hpp) on the CPU:
tests/cpp/test_conditional_plan.cpp includes that header alone — the node's seven errors in the order include/nqe.h states, each shown to
win over the later ones; the typing of every function over every dtype; nesting under and over the other operator nodes; that no tree
that holds the node reaches the stack machine or a fused shape; a zeroed kind-7 node stays INVALID_ARGUMENT and kind 8 is unknown."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_conditional_plan(tmp_path):
    exe = str(tmp_path / "test_conditional_plan")
    src = os.path.join(ROOT, "tests", "cpp", "test_conditional_plan.cpp")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-I", os.path.join(ROOT, "naive_query_engine_amd", "csrc"), src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "conditional plan ok" in out.stdout, out.stdout + out.stderr
