"""The dynamic-LDS layouts of the partitioned aggregate (naive_query_engine_amd/csrc/aggregate_partition_layout.hpp: what the kernels
carve their shared memory by and the host sizes it by) on the CPU: tests/cpp/test_partition_layout.cpp includes that header alone,
is compiled with g++ and run."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_partition_layout(tmp_path):
    exe = str(tmp_path / "test_partition_layout")
    src = os.path.join(ROOT, "tests", "cpp", "test_partition_layout.cpp")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "naive_query_engine_amd", "csrc"), src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "partition layout ok" in out.stdout, out.stdout + out.stderr
