"""The host analysis of nqe_window_execute_ex (naive_query_engine_amd/csrc/window_ex_plan.hpp: the argument checks in their order, the
clamping and classification of ROWS BETWEEN frames, the grouping by (value column, width), and the position arithmetic the emit
kernels call — win_frame_pieces by brute force against the frame's own index list, win_ntile_bucket against SQL's rule) on the CPU:
tests/cpp/test_window_ex_plan.cpp includes that header alone, is compiled with g++ and run."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_window_ex_plan(tmp_path):
    exe = str(tmp_path / "test_window_ex_plan")
    src = os.path.join(ROOT, "tests", "cpp", "test_window_ex_plan.cpp")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-I", os.path.join(ROOT, "naive_query_engine_amd", "csrc"), src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "window ex plan ok" in out.stdout, out.stdout + out.stderr
