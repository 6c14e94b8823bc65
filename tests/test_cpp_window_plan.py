"""The host analysis of the window operator as the first entry sees it (plan_window of naive_query_engine_amd/csrc/window_ex_plan.hpp, the
adapter onto plan_window_ex: the argument checks in their order, the distinct value columns and their scan operators, the position
arrays; window_plan.hpp: the tile and carry counts) on the CPU: tests/cpp/test_window_plan.cpp includes window_plan.hpp alone (which
ends by including the analysis), is compiled with g++ and run."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_window_plan(tmp_path):
    exe = str(tmp_path / "test_window_plan")
    src = os.path.join(ROOT, "tests", "cpp", "test_window_plan.cpp")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-I", os.path.join(ROOT, "naive_query_engine_amd", "csrc"), src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "window plan ok" in out.stdout, out.stdout + out.stderr
